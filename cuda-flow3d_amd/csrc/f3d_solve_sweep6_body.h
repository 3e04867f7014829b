// The body of the one-sweep kernels k_sweep6 and k_last_sweep_flow, included INSIDE each of them (f3d_solve.hip).
//
// Text, not a device function, on purpose: a function is optimised on its own before it is inlined (its arguments opaque pointers, its
// loops unrolled, its lambdas folded in), and k_sweep6 built that way came out with another schedule and register assignment although
// no statement had changed -- which moves the stamp of the solver kernels' machine code that the counter record is held to
// (bench.solver_kernel_stamp, tests/test_abi.py).  Included as text, k_sweep6 compiles to the bytes it had before.
//
// The including kernel provides: its parameters (SolveArgs a, F3dGeo g, int zchunk, ntx, nty, n_tiles, xcd_remap), TY (rows per
// workgroup), ABLATE (timing experiments only, results are wrong: 1 = no arithmetic, 2 = no halo traffic, 3 = no LDS exchange) and
// kAddFlow: false stores the new increments du', dv', dw'; true stores u + du', v + dv', w + dw' (one binary32 add each, what f3d_add
// makes of them: the last sweep of a level).
  __shared__ float img[2][kNL][TY + 2][kLanes];  // face image of the current plane, double buffered
  __shared__ float hrow[kRing][2][9][kLanes];      // raw y-halo rows (edge waves), by LDS-DMA
  __shared__ float hcol[kRing][TY][kLanes];      // raw x-halo values of a row: [array] left, [32 + array] right

  int tile = static_cast<int>(blockIdx.x);
  if (xcd_remap) {
    const int per_xcd = (n_tiles + 7) / 8;
    tile = (tile % 8) * per_xcd + tile / 8;
  }
  if (tile >= n_tiles) return;
  const int tx = tile % ntx;
  const int ty = (tile / ntx) % nty;
  const int tz = tile / (ntx * nty);

  const int lane = threadIdx.x;
  const int r = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  const int z0 = g.z_lo + tz * zchunk;
  const int z1 = min(z0 + zchunk, g.z_hi);
  const int y0 = ty * TY;
  const int y = y0 + r;
  const int yy = f3d_clampi(f3d_mir(y, g.H), 0, g.H - 1);
  const int x = tx * kLanes + lane;
  const int xi = f3d_clampi(f3d_mir(x, g.W), 0, g.W - 1);
  const unsigned xb = static_cast<unsigned>(xi) * 4u;
  const bool owner = x < g.W && y < g.H;
  const int side = lane < 32 ? 0 : 1;
  const int xh = f3d_clampi(f3d_mir(side == 0 ? tx * kLanes - 1 : tx * kLanes + kLanes, g.W), 0, g.W - 1);
  const bool edge = (r == 0) || (r == TY - 1);
  const int which = r == 0 ? 0 : 1;
  const int yh_row = f3d_clampi(f3d_mir(r == 0 ? y0 - 1 : y0 + TY, g.H), 0, g.H - 1);
  const int lds_halo = r == 0 ? 0 : TY + 1;

  // array bases moved to the first plane this chunk touches: every byte offset below is small and positive
  const int zb = z0 > 0 ? z0 - 1 : 0;
  const size_t base_off = f3d_row(g, 0, zb);
  const unsigned plane_b = static_cast<unsigned>(g.Hc) * static_cast<unsigned>(g.pitch) * 4u;
  const unsigned row_b = static_cast<unsigned>(g.pitch) * 4u;
  constexpr int kOrder[9] = {F0, F1, U, V, Wf, DU, DV, DW, PHI};  // order inside the halo rings
  const float* base[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) base[i] = a.in[i] + base_off;
  float* obase[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) obase[i] = a.out[i] + base_off;
  // lane i (and 32 + i), i < 9, gathers the x-halo of array kOrder[i]: its own 64-bit base
  const bool col_lane = (lane & 31) < 9;
  const float* lane_base = base[0];
#pragma unroll
  for (int i = 1; i < 9; ++i)
    if ((lane & 31) == i) lane_base = base[kOrder[i]];
  lane_base += xh;

  auto rowoff = [&](int yrow, int zz) {
    return static_cast<unsigned>(__builtin_amdgcn_readfirstlane(
        static_cast<int>(static_cast<unsigned>(zz - zb) * plane_b + static_cast<unsigned>(yrow) * row_b)));
  };
  auto load_plane = [&](PlaneRegs& p, int zz) {
    const unsigned off = xb + rowoff(yy, zz);
    p.f0 = gld(base[F0], off);
    p.f1 = gld(base[F1], off);
    p.u = gld(base[U], off);
    p.v = gld(base[V], off);
    p.w = gld(base[Wf], off);
    p.su = gld(base[DU], off);
    p.dv = gld(base[DV], off);
    p.dw = gld(base[DW], off);
    p.phi = gld(base[PHI], off);
    p.ksi = gld(base[9], off);
  };
  auto dma_halos = [&](int zz) {  // 1 instruction per wave + 9 for the two edge waves
    const int slot = zz & (kRing - 1);
    if (col_lane) gld_lds_lane(lane_base + (rowoff(yy, zz) >> 2), &hcol[slot][r][0]);
    if (edge) {
      const unsigned off = xb + rowoff(yh_row, zz);
#pragma unroll
      for (int i = 0; i < 9; ++i) gld_lds(base[kOrder[i]], off, &hrow[slot][which][i][0]);
    }
  };
  auto ring_row = [&](PlaneRegs& p, int slot) {
    const float* d = &hrow[slot][which][0][lane];
    p.f0 = d[0 * kLanes]; p.f1 = d[1 * kLanes]; p.u = d[2 * kLanes]; p.v = d[3 * kLanes]; p.w = d[4 * kLanes];
    p.su = d[5 * kLanes]; p.dv = d[6 * kLanes]; p.dw = d[7 * kLanes]; p.phi = d[8 * kLanes];
  };
  auto ring_col = [&](PlaneRegs& p, int slot) {
    const float* d = &hcol[slot][r][side * 32];
    p.f0 = d[0]; p.f1 = d[1]; p.u = d[2]; p.v = d[3]; p.w = d[4]; p.su = d[5]; p.dv = d[6]; p.dw = d[7]; p.phi = d[8];
  };

  // write the face image of a finished plane (own row, and the halo row an edge wave keeps in its ring) into buffer nb
  auto publish = [&](const PlaneRegs& pl, int nb, int ring_slot) {
    const Face6 f = plane_face(pl);
#pragma unroll
    for (int i = 0; i < kNL; ++i) img[nb][i][r + 1][lane] = f.v[i];
    if (edge) {
      PlaneRegs Hc;
      ring_row(Hc, ring_slot);
      plane_finish(Hc);
      const Face6 hf = plane_face(Hc);
#pragma unroll
      for (int i = 0; i < kNL; ++i) img[nb][i][lds_halo][lane] = hf.v[i];
    }
  };

  // M, C, P: finished planes z-1, z, z+1.  Q1: raw plane z+2, requested one step ago.  Q2: receives plane z+3.
  auto step = [&](auto full, const PlaneRegs& M, const PlaneRegs& C, const PlaneRegs& P, PlaneRegs& Q1, PlaneRegs& Q2, int z) {
    constexpr bool FULL = decltype(full)::value;
    const bool row3 = FULL || z + 3 <= z1;   // plane z+3 is somebody's z-neighbour
    const bool halo3 = FULL || z + 3 < z1;   // plane z+3 is computed by this chunk
    if (row3) load_plane(Q2, f3d_mir(z + 3, g.D));
    if (halo3 && ABLATE != 2) dma_halos(z + 3);

    const int b = z & 1;
    const int slot = z & (kRing - 1);
    const Face6 cf = plane_face(C);
    if (ABLATE != 3) __syncthreads();  // the image of plane z is complete: it was written during step z-1 (or the prologue)

    Face6 ym, yp, xm, xp;
#pragma unroll
    for (int i = 0; i < kNL; ++i) {
      ym.v[i] = img[b][i][r][lane];
      yp.v[i] = img[b][i][r + 2][lane];
    }
    PlaneRegs X;
    ring_col(X, slot);
    // Publish the NEXT plane now, off the critical path of the next barrier: buffer b^1 was last read during step z-1,
    // i.e. before the barrier every wave has just passed.
    if ((FULL || z + 1 < z1) && ABLATE != 3) publish(P, b ^ 1, (z + 1) & (kRing - 1));
    plane_finish(X);
    const Face6 xf = plane_face(X);
#pragma unroll
    for (int i = 0; i < kNL; ++i) {
      xm.v[i] = lane_left_or(cf.v[i], xf.v[i]);
      xp.v[i] = lane_right_or(cf.v[i], xf.v[i]);
    }
    float r_du, r_dv, r_dw;
    if (ABLATE == 1) {
      r_du = xm.v[0] + xp.v[1] + ym.v[2] + yp.v[3] + M.su + P.sv + C.ksi;
      r_dv = xm.v[4] + xp.v[5] + ym.v[0] + yp.v[1] + M.f0 + P.f1 + C.u;
      r_dw = xm.v[2] + xp.v[3] + ym.v[4] + yp.v[5] + M.phi + P.phi + C.dv + C.dw + C.v + C.w;
    } else {
      sweep_voxel_s(xm, xp, ym, yp, plane_face(M), plane_face(P), cf.v, C.u, C.v, C.w, C.dv, C.dw, C.ksi, a.hx, a.hy, a.hz,
                    a.p0, x < g.W - 1, x > 0, y < g.H - 1, y > 0, z < g.D - 1, z > 0, r_du, r_dv, r_dw);
    }
    asm volatile("" ::"v"(r_du), "v"(r_dv), "v"(r_dw));
    __builtin_amdgcn_sched_barrier(0);
    // All that was requested BEFORE this step must have landed (plane z+2, its halos, the last stores); what this step
    // requested stays in flight: the counter retires in order, so allow exactly this step's loads.
    if (FULL && ABLATE == 2) {
      F3D_WAIT_PLANE(10, Q1);
    } else if (FULL) {
      if (edge) F3D_WAIT_PLANE(20, Q1);  // 10 row + 1 column gather + 9 halo-row loads
      else F3D_WAIT_PLANE(11, Q1);
    } else {
      F3D_WAIT_PLANE(0, Q1);
    }
    if (FULL || z + 2 <= z1) plane_finish(Q1);
    __builtin_amdgcn_sched_barrier(0);
    if (owner) {
      const unsigned off = xb + rowoff(yy, z);
      gst(obase[0], off, kAddFlow ? C.u + r_du : r_du);
      gst(obase[1], off, kAddFlow ? C.v + r_dv : r_dv);
      gst(obase[2], off, kAddFlow ? C.w + r_dw : r_dw);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  PlaneRegs A, B, C, D, E;
  E = PlaneRegs{};
  D = PlaneRegs{};
  load_plane(A, f3d_mir(z0 - 1, g.D));
  load_plane(B, z0);
  load_plane(C, f3d_mir(z0 + 1, g.D));
  if (z0 + 2 <= z1) load_plane(D, f3d_mir(z0 + 2, g.D));
  dma_halos(z0);
  if (z0 + 1 < z1) dma_halos(z0 + 1);
  if (z0 + 2 < z1) dma_halos(z0 + 2);
  F3D_WAIT_PLANE(0, A);
  F3D_WAIT_PLANE(0, B);
  F3D_WAIT_PLANE(0, C);
  F3D_WAIT_PLANE(0, D);
  plane_finish(A);
  plane_finish(B);
  plane_finish(C);
  __syncthreads();  // DMA-written rings are visible
  publish(B, z0 & 1, z0 & (kRing - 1));
  __builtin_amdgcn_sched_barrier(0);
  int z = z0;
  for (; z + 7 < z1; z += 5) {
    step(std::true_type{}, A, B, C, D, E, z);
    step(std::true_type{}, B, C, D, E, A, z + 1);
    step(std::true_type{}, C, D, E, A, B, z + 2);
    step(std::true_type{}, D, E, A, B, C, z + 3);
    step(std::true_type{}, E, A, B, C, D, z + 4);
  }
  for (; z < z1; z += 5) {
    step(std::false_type{}, A, B, C, D, E, z);
    if (z + 1 < z1) step(std::false_type{}, B, C, D, E, A, z + 1);
    if (z + 2 < z1) step(std::false_type{}, C, D, E, A, B, z + 2);
    if (z + 3 < z1) step(std::false_type{}, D, E, A, B, C, z + 3);
    if (z + 4 < z1) step(std::false_type{}, E, A, B, C, D, z + 4);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores issued by hand
