// f3d_subset_match_table's and f3d_subset_match_layout's host code (cuda-flow3d_amd/host/subset_match.cpp) as a program of its own,
// for a build with -fsanitize=address,undefined: tests/test_subset_match_cpu.py writes the cases, this program works on heap blocks of
// exactly the size the interface names, and the test compares the rows with tests/subset_match_ref.py byte for byte.
//
//   subset_match_table_main table IN OUT
// IN:  int32 ox, oy, oz, step, nx, ny, nz, window, has_compare, 0; float64 min_zncc; nodes * 144 bytes of records; 3 * nodes float32
//      when has_compare.   OUT: nodes * 96 bytes of rows, then the summary (12 uint64, 4 float64).
//   subset_match_table_main layout WIDTH HEIGHT DEPTH STEP WINDOW      prints the eight words of the grid
//   subset_match_table_main sizes                                      prints sizeof record, node, summary, info, grid
// Exit 0 done, 3 refused (the message on stdout, OUT not written), 2 on a malformed call or file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../cuda-flow3d_amd/host/subset_match.cpp"

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  const std::string what = argv[1];
  if (what == "sizes") {
    std::printf("%zu %zu %zu %zu %zu\n", sizeof(f3d_subset_match_record), sizeof(f3d_subset_match_node), sizeof(f3d_subset_match_summary),
                sizeof(f3d_subset_match_info), sizeof(f3d_subset_match_grid));
    return 0;
  }
  if (what == "layout") {
    if (argc != 7) return 2;
    f3d_subset_match_grid grid;
    std::memset(&grid, 0xAB, sizeof(grid));
    std::string why;
    if (!LayoutSubsetMatch(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                           std::atoi(argv[5]), std::atoi(argv[6]), &grid, &why)) {
      const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&grid);
      for (size_t i = 0; i < sizeof(grid); ++i)
        if (bytes[i] != 0xAB) return 4;
      std::printf("refused: %s\n", why.c_str());
      return 3;
    }
    std::printf("%d %d %d %d %d %d %d %d\n", grid.ox, grid.oy, grid.oz, grid.step, grid.nx, grid.ny, grid.nz, grid.window);
    return 0;
  }
  if (what != "table" || argc != 4) return 2;
  std::FILE* in = std::fopen(argv[2], "rb");
  if (!in) return 2;
  int head[10];
  double min_zncc;
  if (std::fread(head, sizeof(int), 10, in) != 10 || std::fread(&min_zncc, sizeof(double), 1, in) != 1) return 2;
  const f3d_subset_match_grid grid = {head[0], head[1], head[2], head[3], head[4], head[5], head[6], head[7]};
  const bool has_compare = head[8] != 0;
  // the sizes the file holds, which for a grid that is refused are not the grid's
  size_t nodes = 0;
  {
    const long at = std::ftell(in);
    std::fseek(in, 0, SEEK_END);
    const long rest = std::ftell(in) - at;
    std::fseek(in, at, SEEK_SET);
    const size_t per_node = sizeof(f3d_subset_match_record) + (has_compare ? 3 * sizeof(float) : 0);
    if (rest < 0 || static_cast<size_t>(rest) % per_node) return 2;
    nodes = static_cast<size_t>(rest) / per_node;
  }
  std::unique_ptr<f3d_subset_match_record[]> records(new f3d_subset_match_record[nodes]);
  std::unique_ptr<float[]> held[3];
  const float* compare[3] = {nullptr, nullptr, nullptr};
  std::unique_ptr<f3d_subset_match_node[]> rows(new f3d_subset_match_node[nodes]);
  if (std::fread(static_cast<void*>(records.get()), sizeof(f3d_subset_match_record), nodes, in) != nodes) return 2;
  for (int c = 0; c < 3 && has_compare; ++c) {
    held[c].reset(new float[nodes]);
    if (std::fread(held[c].get(), sizeof(float), nodes, in) != nodes) return 2;
    compare[c] = held[c].get();
  }
  std::fclose(in);
  std::memset(static_cast<void*>(rows.get()), 0xAB, nodes * sizeof(f3d_subset_match_node));
  if (grid.nx > 0 && grid.ny > 0 && grid.nz > 0) {
    const unsigned long long want = static_cast<unsigned long long>(grid.nx) * grid.ny * grid.nz;
    if (want <= F3D_SUBSET_MATCH_MAX_NODES && want != nodes) return 2;
  }
  f3d_subset_match_summary summary;
  std::string why;
  if (!TableSubsetMatch(records.get(), &grid, min_zncc, has_compare ? compare : nullptr, rows.get(), &summary, &why)) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(rows.get());
    for (size_t i = 0; i < nodes * sizeof(f3d_subset_match_node); ++i)
      if (bytes[i] != 0xAB) return 4;
    std::printf("refused: %s\n", why.c_str());
    return 3;
  }
  // the same again without a summary
  std::unique_ptr<f3d_subset_match_node[]> again(new f3d_subset_match_node[nodes]);
  if (!TableSubsetMatch(records.get(), &grid, min_zncc, has_compare ? compare : nullptr, again.get(), nullptr, &why)) return 4;
  if (std::memcmp(static_cast<const void*>(rows.get()), static_cast<const void*>(again.get()), nodes * sizeof(f3d_subset_match_node))) return 4;
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!out) return 2;
  std::fwrite(static_cast<const void*>(rows.get()), sizeof(f3d_subset_match_node), nodes, out);
  std::fwrite(&summary, sizeof(summary), 1, out);
  std::fclose(out);
  std::printf("ok\n");
  return 0;
}
