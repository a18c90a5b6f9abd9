// Body of the persistent interior-point kernels (ipm_persistent.hip), included inside
// ipm_solve_kernel and ipm_solve_params_kernel: the text between the braces, moved here unchanged
// so that both kernels compile the same statements on their own by-value arguments.  In scope at
// the point of inclusion: the template parameters KIND, NX, NU, WPS, RESUME, XLDS, STRUCT, SPEC (the
// params kernel fixes STRUCT = true, SPEC = 1) and the arguments prm, w, mode, terminal, bp0,
// max_solves.  Not a stand-alone header (no include guard on purpose).
  static_assert(SPEC == 1 || XLDS, "speculative waves keep x, u in LDS");
  // one wave (= one 64-thread workgroup) per trajectory -- SPEC waves with SPEC > 1; w.order: the
  // launch order (a permutation)
  const int b = w.order ? w.order[blockIdx.x] : (int)blockIdx.x;
  const int l = SPEC > 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;  // lane = chunk owner
  const int wv = SPEC > 1 ? (int)(threadIdx.x >> 6) : 0;                 // candidate of this wave
  const bool lead = (l == 0) && (wv == 0);  // writes the trajectory's results
  (void)lead;
  if (b < 0 || b >= w.Bt) return;  // an out-of-range order entry solves nothing (never faults)
  constexpr int KD = kd_width<NX, NU>();
  Fam<KIND, NX, NU> f(prm);
  using BS = BlockStruct<KIND, NX, NU, STRUCT>;
  constexpr int VA = BS::template nv<BF_A>(), VB = BS::template nv<BF_B>();
  constexpr int VQ = BS::template nv<BF_Q>(), VR = BS::template nv<BF_R>(), VM = BS::template nv<BF_M>();
  const int N = w.N;
  const Chunks ch(N, PL);
  const int start = ch.start(l), len = ch.len(l), cmax = ch.cmax;
  const bool last = (l == PL - 1);
  // Stage pairs: two stages per pass through the per-stage loops (linearise, costate + blocks,
  // trial), both loaded before either is computed, so their independent transcendental chains
  // (sincos, divisions, log) interleave.  Needs the 1-wave-per-SIMD register budget; the trip
  // count follows the wave-uniform chunk bound cmax (lanes past their own chunk compute a clamped
  // duplicate stage and discard it).
  const bool pair = (WPS == 1) && cmax >= 2;
  auto clampk = [&](int k) { return k < N - 1 ? k : N - 1; };
  double* const Xg = w.x + (size_t)b * (N + 1) * NX;
  double* const Ug = w.u + (size_t)b * N * NU;
  extern __shared__ __attribute__((aligned(16))) double noc_smem[];
  double* const X = XLDS ? noc_smem + xlds_off<NX, NU>(N, SPEC, wv) : Xg;
  double* const U = XLDS ? noc_smem + xlds_off<NX, NU>(N, SPEC, wv) + (N + 1) * NX : Ug;
  if constexpr (XLDS) {  // the workspace's x (a resume point's states) and u into LDS
    for (int i = l; i < (N + 1) * NX; i += 64) X[i] = Xg[i];
    for (int i = l; i < N * NU; i += 64) U[i] = Ug[i];
    wave_fence();
  }
  const double* slot = lds_slots<NX, NU, PL>(N);

  KKTArgs a{};
  a.N = N;
  a.B = w.Bt;
  a.mode = MODE_FULL;
  a.A = w.A; a.Bm = w.B; a.Q = w.Q; a.R = w.R; a.M = w.M; a.r = w.r; a.P = w.P; a.reg = w.reg;
  a.pred = w.pred; a.feasible = w.feasible;
  a.tiled = 1;
  a.lds_out = 1;  // dx, du stay in LDS (a.dx = a.du = NULL): the trial reads them there
  SpecIO* const io = SPEC > 1 ? spec_io<NX, NU>(N, SPEC, wv) : nullptr;
  if constexpr (SPEC > 1) {  // this wave's candidate: reg, pred, feasible in its LDS record
    a.reg = &io->reg;
    a.pred = &io->pred;
    a.feasible = &io->feasible;
  }

  IpmState sol;  // the solver state and its accept rule / barrier schedule: ipm_schedule.h
  sol.init(bp0);
  bool capped = false;
  int phase = NOC_PHASE_DONE;     // the resume point a capped launch leaves in the workspace
  int entry = NOC_PHASE_ROLLOUT;  // RESUME: where this launch starts
  if constexpr (RESUME) {
    sol.load(w, b);
    entry = resume_phase(w.phase[b]);
    if (entry == NOC_PHASE_DONE) return;  // uniform over the wave
  } else {
    if (lead && w.repeats) w.repeats[b] = 0;
  }

#ifdef NOC_PERSIST_PROFILE
  long long t_prev = clock64();
  if (lead && b < kTrajStamps) g_traj_times[b][0] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  // lc_fresh: the workspace's stage costs (w.lc) already belong to the current (x, u) -- the last
  // trial wrote them, and it was taken -- so the next linearisation skips f.stage_cost (the
  // trial evaluated the same function on the same doubles: x + dx is the update's own sum).  False
  // at every launch start (a resume may follow the per-phase driver, whose trial does not write
  // w.lc) and after every rollout (new barrier parameter).
  bool lc_fresh = false;
  for (;;) {  // ---------------- barrier stages (P:228-254) ----------------
    // rollout x_{k+1} = f(x_k, u_k) (noc/utils.py:57-63, P:133): every lane runs the recurrence
    // redundantly with u_k broadcast by readlane; lane t stores the states of block step t
    wave_fence();  // u was last written chunk-wise by the trials
    if (!RESUME || entry == NOC_PHASE_ROLLOUT) {
      double x[NX];
      NOC_UNROLL for (int i = 0; i < NX; ++i) x[i] = w.x0[(size_t)b * NX + i];
      if (l < NX) X[l] = x[l];
      for (int base = 0; base < N; base += 64) {
        const int k = base + l;
        double uk[NU];
        NOC_UNROLL for (int j = 0; j < NU; ++j) uk[j] = (k < N) ? U[(size_t)k * NU + j] : 0.0;
        double mine[NX];
        NOC_UNROLL for (int i = 0; i < NX; ++i) mine[i] = 0.0;
        const int cnt = (N - base < 64) ? (N - base) : 64;
        for (int t = 0; t < cnt; ++t) {
          double ut[NU], xn[NX];
          NOC_UNROLL for (int j = 0; j < NU; ++j) ut[j] = readlane_d(uk[j], t);
          f.step(x, ut, xn);
          NOC_UNROLL for (int i = 0; i < NX; ++i) {
            x[i] = xn[i];
            mine[i] = (l == t) ? xn[i] : mine[i];
          }
        }
        if (k < N) NOC_UNROLL for (int i = 0; i < NX; ++i) X[(size_t)(k + 1) * NX + i] = mine[i];
      }
    }
    wave_fence();  // states of every stage visible to their chunk owners
    NOC_PHASE(0);
    lc_fresh = false;
    // A SOLVE resume (a retry on the current point) recomputes the blocks from the workspace's
    // states -- the same doubles the capped launch had; the workspace blocks may be another
    // driver's layout (dense / compact) -- and keeps the solver state it left (cost, |Hu|,
    // ||cu||, the retry counter), like the wide kernel (ipm_wide.hip)
    bool relinearize = true;
    bool keep_state = RESUME && entry == NOC_PHASE_SOLVE;
    if constexpr (RESUME) entry = NOC_PHASE_ROLLOUT;
    bool stage_done = false;
    while (!stage_done) {  // ---------------- Newton iterations (P:127-225) ----------------
      const bool relinearized = relinearize;  // uniform over the workgroup
      if (relinearize) {
        // linearise the own chunk (P:13-28): A = fx, B = fu, cx, cu, stage cost
        struct LinOut {
          double fx[NX * NX], fu[NX * NU], cx[NX], cu[NU], lc;
        };
        auto lin_compute = [&](const double* x, const double* u, LinOut& o) {
          f.jac(x, u, o.fx, o.fu);
          BS::template fold_consts<BF_A>(prm, o.fx);  // structural entries as literals / parameters
          BS::template fold_consts<BF_B>(prm, o.fu);
          f.stage_grad(x, u, sol.bp, o.cx, o.cu);
          if (!lc_fresh) o.lc = f.stage_cost(x, u, sol.bp);  // uniform over the wave
        };
        auto lin_store = [&](int j, const LinOut& o) {  // compact A, B: variable entries only
          double va[VA > 0 ? VA : 1], vb[VB > 0 ? VB : 1];
          BS::template compress<BF_A>(o.fx, va);
          BS::template compress<BF_B>(o.fu, vb);
          if constexpr (VA > 0) tstore<VA, PL>(w.A, b, j, l, cmax, va);
          if constexpr (VB > 0) tstore<VB, PL>(w.B, b, j, l, cmax, vb);
          if (!lc_fresh) tstore<1, PL>(w.lc, b, j, l, cmax, &o.lc);
        };
        auto load_xu = [&](int k, double* x, double* u) {
          gload<NX>(X + (size_t)k * NX, x);
          NOC_UNROLL for (int i = 0; i < NU; ++i) u[i] = U[(size_t)k * NU + i];
        };
        // The costates are a reverse affine scan (C:34-54) fused with the LQ blocks (P:31-42).
        // Its in-chunk fold (G, g) <- (A' G, cx + A' g) runs inside the linearisation, which
        // walks the chunk backwards for it, on the A, cx it has just computed -- the same
        // operations in the same order as a separate pass reading them back from the workspace,
        // without that pass's loads (the solve moves ~6.5 TB/s at c3).
        Mat<NX, NX> G;
        Vec<NX> g;
        set_identity(G);
        set_zero(g);
        auto fold = [&](const LinOut& o, bool valid) {
          Mat<NX, NX> Gn;
          Vec<NX> gn;
          NOC_UNROLL for (int i = 0; i < NX; ++i) {
            double t = o.cx[i];
            NOC_UNROLL for (int m = 0; m < NX; ++m) if (BS::nzA(m, i)) t += o.fx[m * NX + i] * g[m];
            gn[i] = t;
            NOC_UNROLL for (int jj = 0; jj < NX; ++jj) {
              double u = 0.0;
              NOC_UNROLL for (int m = 0; m < NX; ++m) if (BS::nzA(m, i)) u += o.fx[m * NX + i] * G(m, jj);
              Gn(i, jj) = u;
            }
          }
          NOC_UNROLL for (int i = 0; i < NX * NX; ++i) G.v[i] = valid ? Gn.v[i] : G.v[i];
          NOC_UNROLL for (int i = 0; i < NX; ++i) g.v[i] = valid ? gn.v[i] : g.v[i];
        };
        if (pair) {  // descending pairs over the wave-uniform chunk bound: loads, then both
                     // computations, then the stores and the fold (one basic block of work)
          for (int j = cmax - 1; j >= 0; j -= 2) {
            double x0[NX], u0[NU], x1[NX], u1[NU];
            load_xu(clampk(start + j), x0, u0);
            load_xu(clampk(start + (j - 1 >= 0 ? j - 1 : j)), x1, u1);
            const bool v0 = j < len, v1 = j - 1 >= 0 && j - 1 < len;
            LinOut o0, o1;
            lin_compute(x0, u0, o0);
            lin_compute(x1, u1, o1);
            if (v0) lin_store(j, o0);
            if (v1) lin_store(j - 1, o1);
            fold(o0, v0);
            fold(o1, v1);
          }
        } else {
          for (int j = len - 1; j >= 0; --j) {
            double x[NX], u[NU];
            load_xu(start + j, x, u);
            LinOut o;
            lin_compute(x, u, o);
            lin_store(j, o);
            fold(o, true);
          }
        }
        NOC_PHASE(1);
        const double* xN = X + (size_t)N * NX;
        double lamN[NX];
        NOC_T0(t_cs);
        f.final_grad(xN, lamN);  // grad(final_cost) (C:35)
        if (last) {
          NOC_UNROLL for (int i = 0; i < NX; ++i) {
            double t = g[i];
            NOC_UNROLL for (int m = 0; m < NX; ++m) t += G(i, m) * lamN[m];
            g[i] = t;
          }
          set_zero(G);
        }
#pragma unroll 1
        for (int d = 1; d < PL; d <<= 1) {
          Mat<NX, NX> G2;
          Vec<NX> g2;
          shfl_down_arr<NX * NX>(G.v, G2.v, d, PL);
          shfl_down_arr<NX>(g.v, g2.v, d, PL);
          Mat<NX, NX> Gn;
          NOC_UNROLL for (int i = 0; i < NX; ++i) {
            double t = g[i];
            NOC_UNROLL for (int m = 0; m < NX; ++m) t += G(i, m) * g2[m];
            g[i] = t;
            NOC_UNROLL for (int jj = 0; jj < NX; ++jj) {
              double u = 0.0;
              NOC_UNROLL for (int m = 0; m < NX; ++m) u += G(i, m) * G2(m, jj);
              Gn(i, jj) = u;
            }
          }
          G = Gn;
        }
        // The costates stay in registers: the solve does not store lambda to the workspace (a
        // strided 8 * nx bytes per stage and lane, c3 ipm_solve -2.7 %, profiles/r05/lam_store/)
        double lam[NX];
        shfl_down_arr<NX>(g.v, lam, 1, PL);
        if (last) NOC_UNROLL for (int i = 0; i < NX; ++i) lam[i] = lamN[i];
        NOC_SUB(7, t_cs);
        double csum = 0.0, hmax = 0.0, g2s = 0.0;
        // One stage of the costate sweep fused with its LQ blocks.  `valid` = false computes on a
        // clamped duplicate stage and leaves lambda, the sums and memory untouched (selects, not
        // branches, so a pair of stages stays one basic block).
        struct StageIn {
          double A[NX * NX], Bm[NX * NU], cx[NX], cu[NU], lc, x[NX], u[NU];
        };
        auto load_in = [&](int j, StageIn& in) {
          // 0 <= j < cmax: every lane's tiled slots exist up to cmax; for a slot past the lane's
          // own chunk the data are a discarded duplicate (x, u clamped into the horizon)
          double va[VA > 0 ? VA : 1], vb[VB > 0 ? VB : 1];
          if constexpr (VA > 0) tload<VA, PL>(w.A, b, j, l, cmax, va);
          if constexpr (VB > 0) tload<VB, PL>(w.B, b, j, l, cmax, vb);
          BS::template expand<BF_A>(prm, va, in.A);
          BS::template expand<BF_B>(prm, vb, in.Bm);
          tload<1, PL>(w.lc, b, j, l, cmax, &in.lc);
          load_xu(clampk(start + j), in.x, in.u);
          // cx, cu re-evaluated (the linearisation's values bit for bit) instead of stored and read
          // back: a workspace round trip of nx + nu doubles per stage against one stage_grad
          f.stage_grad(in.x, in.u, sol.bp, in.cx, in.cu);
        };
        // LQ blocks at lambda_{k+1} (P:35-37): Q = cxx + l.fxx, R = cuu + l.fuu, M = cxu + l.fxu;
        // ru_k = cu_k + fu_k' lambda_{k+1} (P:34); then lambda_k = cx_k + fx_k' lambda_{k+1}
        struct StageOut {
          Sym<NX> Qs;
          Sym<NU> Rs;
          double M[NX * NU], rr[NU], lam[NX];
        };
        auto cost_compute = [&](const StageIn& in, bool valid, StageOut& o) {
          double Q[NX * NX], R[NU * NU];
          f.stage_hess(in.x, in.u, sol.bp, Q, R, o.M);
          f.add_hess_l(in.x, in.u, lam, Q, R, o.M);
          BS::template fold_consts<BF_M>(prm, o.M);
          NOC_UNROLL for (int i = 0; i < NX; ++i)
            NOC_UNROLL for (int jj = i; jj < NX; ++jj) o.Qs(i, jj) = (i == jj) ? Q[i * NX + i] : 0.5 * (Q[i * NX + jj] + Q[jj * NX + i]);
          NOC_UNROLL for (int i = 0; i < NU; ++i)
            NOC_UNROLL for (int jj = i; jj < NU; ++jj) o.Rs(i, jj) = (i == jj) ? R[i * NU + i] : 0.5 * (R[i * NU + jj] + R[jj * NU + i]);
          BS::template fold_consts<BF_Q>(prm, o.Qs.v);
          BS::template fold_consts<BF_R>(prm, o.Rs.v);
          NOC_UNROLL for (int jj = 0; jj < NU; ++jj) {
            double r = in.cu[jj];
            NOC_UNROLL for (int i = 0; i < NX; ++i) if (BS::nzB(i, jj)) r += in.Bm[i * NU + jj] * lam[i];
            o.rr[jj] = r;
            hmax = valid ? nan_max(hmax, fabs(r)) : hmax;
            g2s = valid ? g2s + in.cu[jj] * in.cu[jj] : g2s;
          }
          NOC_UNROLL for (int i = 0; i < NX; ++i) {
            double t = in.cx[i];
            NOC_UNROLL for (int m = 0; m < NX; ++m) if (BS::nzA(m, i)) t += in.A[m * NX + i] * lam[m];
            o.lam[i] = t;
          }
          csum = valid ? csum + in.lc : csum;
          NOC_UNROLL for (int i = 0; i < NX; ++i) lam[i] = valid ? o.lam[i] : lam[i];
        };
        auto cost_store = [&](int j, const StageIn& in, const StageOut& o) {
          const int k = start + j;
          double vq[VQ > 0 ? VQ : 1], vr[VR > 0 ? VR : 1], vm[VM > 0 ? VM : 1];
          BS::template compress<BF_Q>(o.Qs.v, vq);
          BS::template compress<BF_R>(o.Rs.v, vr);
          BS::template compress<BF_M>(o.M, vm);
          if constexpr (VQ > 0) tstore<VQ, PL>(w.Q, b, j, l, cmax, vq);
          if constexpr (VR > 0) tstore<VR, PL>(w.R, b, j, l, cmax, vr);
          if constexpr (VM > 0) tstore<VM, PL>(w.M, b, j, l, cmax, vm);
          if (terminal == NOC_TERMINAL_STAGE0 && k == 0) {  // XT = Q[0] (P:73), full matrix
            double Q[NX * NX];
            NOC_UNROLL for (int i = 0; i < NX; ++i) NOC_UNROLL for (int jj = 0; jj < NX; ++jj) Q[i * NX + jj] = o.Qs(i, jj);
            gstore<NX * NX>(w.P + (size_t)b * NX * NX, Q);
          }
          tstore<NU, PL>(w.r, b, j, l, cmax, o.rr);
        };
        if (pair) {  // descending pairs over the wave-uniform chunk bound; short lanes skip slots
          for (int j = cmax - 1; j >= 0; j -= 2) {
            StageIn in0, in1;
            load_in(j, in0);
            load_in(j - 1 >= 0 ? j - 1 : j, in1);
            const bool v0 = j < len, v1 = j - 1 >= 0 && j - 1 < len;
            StageOut o0, o1;
            cost_compute(in0, v0, o0);
            cost_compute(in1, v1, o1);
            if (v0) cost_store(j, in0, o0);
            if (v1) cost_store(j - 1, in1, o1);
          }
        } else {
          for (int j = len - 1; j >= 0; --j) {
            StageIn in;
            load_in(j, in);
            StageOut o;
            cost_compute(in, true, o);
            cost_store(j, in, o);
          }
        }
        // lambda at the chunk start := the scan's value g (not this lane's sweep): it is exactly the
        // boundary costate the previous lane used, so every consumer of lambda_k sees one value
        {  // the __shfl_xor butterflies with VALU partners (bit-identical, small_linalg.h)
          const int ln = (int)__lane_id();
          auto add = [](double x, double y) { return x + y; };
          csum = segment_allreduce<PL>(csum, ln, add);
          g2s = segment_allreduce<PL>(g2s, ln, add);
          hmax = segment_allreduce<PL>(hmax, ln, [](double x, double y) { return nan_max(x, y); });
        }
        if (terminal == NOC_TERMINAL_FINAL_COST && last) {  // hessian(final_cost) (S:66)
          double P[NX * NX];
          f.final_hess(xN, P);
          gstore<NX * NX>(w.P + (size_t)b * NX * NX, P);
        }
        if (!keep_state) {
          // total_cost(x, u, bp) (P:142); x_N is the last lane's own (trial) store
          sol.cost = readlane_d(csum + f.final_cost(xN), PL - 1);
          sol.hu = hmax;                                  // max |Hu| (P:158)
          sol.gnorm = sqrt(g2s);                          // ||cu||_F (P:116)
          sol.inner = 0;
        }
        keep_state = false;
        relinearize = false;
      }
      // The candidates of this solve: candidate k is the regularisation the solver reaches after
      // k rejected trials at this point (reg_update, ipm_schedule.h).  SPEC = 1: only k = 0, stored
      // per trajectory as before; SPEC > 1: wave k solves candidate k (its LDS record).
      double c_reg[SPEC];
      {
        double r = sol.rp, ri = sol.rinc;
        NOC_UNROLL for (int k = 0; k < SPEC; ++k) {
          c_reg[k] = candidate_reg(mode, r, sol.gnorm);
          reg_update(mode, false, 0.0, r, ri);
        }
      }
      if constexpr (SPEC == 1) {
        w.reg[b] = c_reg[0];  // every lane stores the same value and reads its own store back
      } else {
        double rw = c_reg[0];
        NOC_UNROLL for (int k = 1; k < SPEC; ++k) rw = (wv == k) ? c_reg[k] : rw;
        io->reg = rw;
      }
      NOC_PHASE(2);
      wave_fence();  // the terminal Hessian (stage-0 lane) and the blocks before the scan
      // SPEC > 1: every wave has written the blocks (the same doubles) and read w.lc before any
      // wave's trial overwrites w.lc (a retry reads neither: no barrier)
      if constexpr (SPEC > 1) {
        if (relinearized) __syncthreads();
      }
      *state_slot<NX, NU>(N, SPEC, wv) = sol;  // park the state (every lane stores the same values)
      // ---------------- KKT solve (par_Newton, P:107-124) ----------------
      // HANDOFF on (phase 3 hands the chunk's first A, B to phase 4 in registers): the two-wave
      // cart-pole instance's scratch 524 -> 560 B/lane, but the solve is bound by its workspace
      // traffic -- c3 ipm_solve -2.4 %, c2 -1 %, bit-identical (profiles/r05/handoff_persist/)
      {
        const CompactSrc<BS, NX, NU, PL> src{a, prm, b, l, cmax, (size_t)b * N};
        kkt_scan_wave_src<NX, NU, PL, false, true, CompactSrc<BS, NX, NU, PL>, ScanOptIO0<(SPEC > 1)>>(a, b, l, src);
      }
      wave_fence();  // pred / feasible written by lane 0
      sol = *state_slot<NX, NU>(N, SPEC, wv);
      NOC_PHASE(3);
      // ---------------- trial point (P:156-175 / S:121-161) ----------------
      // (SPEC > 1: wave 0's trial costs go to w.lc -- the next linearisation's if its candidate is
      // taken; the other waves' are recomputed there, the same doubles)
      NOC_T0(t_tr);
      double tsum = 0.0;
      int ok = 1;
      const bool lc_out = SPEC == 1 || wv == 0;
      auto trial_load = [&](int k, double* xt, double* ut) {
        NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)k * NX + i] + slot[k * KD + i];
        NOC_UNROLL for (int jj = 0; jj < NU; ++jj) ut[jj] = U[(size_t)k * NU + jj] + slot[k * KD + NX + jj];
      };
      if (pair) {  // both stages loaded, then both costs; summed in stage order like trial_kernel
        for (int j = 0; j < cmax; j += 2) {
          double xt0[NX], ut0[NU], xt1[NX], ut1[NU];
          trial_load(clampk(start + j), xt0, ut0);
          trial_load(clampk(start + j + 1), xt1, ut1);
          const double c0 = f.stage_cost(xt0, ut0, sol.bp);
          const double c1 = f.stage_cost(xt1, ut1, sol.bp);
          const bool f0 = f.feasible(xt0, ut0), f1 = f.feasible(xt1, ut1);
          if (j < len) { ok &= f0 ? 1 : 0; tsum += c0; if (lc_out) tstore<1, PL>(w.lc, b, j, l, cmax, &c0); }
          if (j + 1 < len) { ok &= f1 ? 1 : 0; tsum += c1; if (lc_out) tstore<1, PL>(w.lc, b, j + 1, l, cmax, &c1); }
        }
      } else {
        for (int j = 0; j < len; ++j) {
          double xt[NX], ut[NU];
          trial_load(start + j, xt, ut);
          ok &= f.feasible(xt, ut) ? 1 : 0;
          const double c = f.stage_cost(xt, ut, sol.bp);
          tsum += c;
          if (lc_out) tstore<1, PL>(w.lc, b, j, l, cmax, &c);  // the next linearisation's, if taken
        }
      }
      if (last) {
        double xt[NX];
        NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)N * NX + i] + slot[N * KD + i];
        tsum += f.final_cost(xt);
      }
      tsum = wave_sum(tsum);
      const bool traj_ok = __all(ok);
      NOC_SUB(6, t_tr);
      // the candidates' outcomes: new cost (P:159-163, S:126-129), pred, backward feasibility
      double c_new[SPEC], c_pred[SPEC];
      bool c_bwd[SPEC];
      if constexpr (SPEC == 1) {
        c_new[0] = traj_ok ? tsum : INFINITY;
        c_pred[0] = w.pred[b];
        c_bwd[0] = w.feasible[b] != 0;
      } else {
        if (l == 0) io->new_cost = traj_ok ? tsum : INFINITY;
        __syncthreads();  // every candidate's outcome in LDS
        const SpecIO* io0 = spec_io<NX, NU>(N, SPEC, 0);
        NOC_UNROLL for (int k = 0; k < SPEC; ++k) {
          c_new[k] = io0[k].new_cost;
          c_pred[k] = io0[k].pred;
          c_bwd[k] = io0[k].feasible != 0;
        }
      }
      // The accept tests in solve order.  Candidate k > 0 counts only if the solver reaches it:
      // every earlier one rejected without ending the iteration, no stop, no cap, and its
      // regularisation the one the sequential solver would use next (bit for bit) -- so the
      // decisions, counters and iterates are the sequential solver's.
      int winner = -1;
      NOC_UNROLL for (int k = 0; k < SPEC; ++k) {
        if (k > 0 && (stage_done || relinearize || candidate_reg(mode, sol.rp, sol.gnorm) != c_reg[k])) break;
        const AcceptOutcome o = accept_step(sol, mode, c_new[k], c_pred[k], c_bwd[k], w.flags,
                                            max_solves - sol.solves - 1, lead ? &g_dtrace : nullptr, b);
        if (o.rep > 0 && lead && w.repeats) w.repeats[b] += o.rep;
        if (o.take) winner = k;
#ifdef NOC_PERSIST_PROFILE
        if (b == 0 && lead) g_phase_cycles[5] += 1;
#endif
        stage_done = o.stage_done;
        relinearize = o.relinearize;
        if (sol.solves >= max_solves) {  // capped: record where a later launch continues
          capped = true;
          phase = resume_point(stage_done, relinearize, sol.bp, w.flags);
          break;
        }
      }
      if (winner >= 0) {  // x <- x + dx, u <- u + du on the own chunk (its later readers are this lane)
        const double* ws = slot + (winner - wv) * slot_doubles<NX, NU>(N);  // the winner's slots
        for (int j = 0; j < len; ++j) {
          const int k = start + j;
          NOC_UNROLL for (int i = 0; i < NX; ++i) X[(size_t)k * NX + i] += ws[k * KD + i];
          NOC_UNROLL for (int jj = 0; jj < NU; ++jj) U[(size_t)k * NU + jj] += ws[k * KD + NX + jj];
        }
        if (last) NOC_UNROLL for (int i = 0; i < NX; ++i) X[(size_t)N * NX + i] += ws[N * KD + i];
      }
      lc_fresh = winner == 0;  // uniform; candidate 0's trial stored this point's stage costs in w.lc
      __syncthreads();  // the next KKT solve overwrites the LDS slots read above
      NOC_PHASE(4);
      if (capped) break;
    }
    if (capped || !(sol.bp > 1e-4)) break;                      // P:243-245
    if (w.flags & NOC_WS_ONE_STAGE) break;                      // newton_oc: one stage
  }
  if constexpr (XLDS) {  // states and controls back to the workspace (every copy is the same)
    wave_fence();
    if (wv == 0) {
      for (int i = l; i < (N + 1) * NX; i += 64) Xg[i] = X[i];
      for (int i = l; i < N * NU; i += 64) Ug[i] = U[i];
    }
  }
  if (lead) {
    sol.store(w, b, phase);
#ifdef NOC_PERSIST_PROFILE
    if (b < kTrajStamps) g_traj_times[b][1] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  }
