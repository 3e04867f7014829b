// f3d_block_match_solve's host code (cuda-flow3d_amd/host/block_match.cpp) as a program of its own, for a build with
// -fsanitize=address,undefined: tests/test_block_match_cpu.py writes the cases, this program solves them from heap blocks of exactly
// the size the interface names, and the test compares the rows with tests/block_match_ref.py byte for byte.
//
//   block_match_solve_main IN OUT
// IN:  int32 nx, ny, nz, ox, oy, oz, step, window, rx, ry, rz, has_centre; float64 min_zncc; nodes * 32 int32 records;
//      nodes * 3 int32 centres when has_centre.   OUT: nodes * 88 bytes of rows, then the summary (6 uint64).
// Exit 0 solved, 3 refused (the message on stdout, OUT not written), 2 on a malformed file.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../cuda-flow3d_amd/host/block_match.cpp"

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int head[12];
  double min_zncc;
  if (std::fread(head, sizeof(int), 12, in) != 12 || std::fread(&min_zncc, sizeof(double), 1, in) != 1) return 2;
  f3d_block_match_grid grid;
  grid.nx = head[0], grid.ny = head[1], grid.nz = head[2];
  grid.ox = head[3], grid.oy = head[4], grid.oz = head[5];
  grid.step = head[6], grid.window = head[7];
  grid.rx = head[8], grid.ry = head[9], grid.rz = head[10];
  const bool has_centre = head[11] != 0;
  // the sizes the file holds, which for a grid that is refused are not the grid's
  size_t nodes = 0;
  {
    const long at = std::ftell(in);
    std::fseek(in, 0, SEEK_END);
    const long rest = std::ftell(in) - at;
    std::fseek(in, at, SEEK_SET);
    const size_t per_node = sizeof(f3d_block_match_record) + (has_centre ? 3 * sizeof(int) : 0);
    if (rest < 0 || static_cast<size_t>(rest) % per_node) return 2;
    nodes = static_cast<size_t>(rest) / per_node;
  }
  std::unique_ptr<f3d_block_match_record[]> records(new f3d_block_match_record[nodes]);
  std::unique_ptr<int[]> centre(has_centre ? new int[3 * nodes] : nullptr);
  std::unique_ptr<f3d_block_match_node[]> rows(new f3d_block_match_node[nodes]);
  if (std::fread(records.get(), sizeof(f3d_block_match_record), nodes, in) != nodes) return 2;
  if (has_centre && std::fread(centre.get(), 3 * sizeof(int), nodes, in) != nodes) return 2;
  std::fclose(in);
  std::memset(static_cast<void*>(rows.get()), 0xAB, nodes * sizeof(f3d_block_match_node));

  // a grid the solve accepts walks nx ny nz records: the file must hold as many
  if (grid.nx > 0 && grid.ny > 0 && grid.nz > 0) {
    const unsigned long long want = static_cast<unsigned long long>(grid.nx) * grid.ny * grid.nz;
    if (want <= F3D_BLOCK_MATCH_MAX_NODES && want != nodes) return 2;
  }
  f3d_block_match_summary summary;
  std::string why;
  if (!SolveBlockMatch(records.get(), &grid, centre.get(), min_zncc, rows.get(), &summary, &why)) {
    // nothing was written
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(rows.get());
    for (size_t i = 0; i < nodes * sizeof(f3d_block_match_node); ++i)
      if (bytes[i] != 0xAB) return 4;
    std::printf("refused: %s\n", why.c_str());
    return 3;
  }
  // the same again without a summary
  std::unique_ptr<f3d_block_match_node[]> again(new f3d_block_match_node[nodes]);
  if (!SolveBlockMatch(records.get(), &grid, centre.get(), min_zncc, again.get(), nullptr, &why)) return 4;
  if (std::memcmp(static_cast<const void*>(rows.get()), static_cast<const void*>(again.get()), nodes * sizeof(f3d_block_match_node))) return 4;
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(rows.get(), sizeof(f3d_block_match_node), nodes, out);
  std::fwrite(&summary, sizeof(summary), 1, out);
  std::fclose(out);
  std::printf("ok\n");
  return 0;
}
