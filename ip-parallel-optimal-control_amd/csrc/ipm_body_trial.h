// Body of trial_kernel and its per-trajectory-parameter twin (ipm_kernels.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= w.Bt || w.phase[b] != NOC_PHASE_SOLVE) return;  // uniform per wave
  Fam<KIND, NX, NU> f(prm);
  const int N = w.N;
  const double bp = w.bp[b];
  const double* X = w.x + (size_t)b * (N + 1) * NX;
  const double* DX = w.dx + (size_t)b * (N + 1) * NX;
  const double* U = w.u + (size_t)b * N * NU;
  const double* DU = w.du + (size_t)b * N * NU;
  // lane l sums the stages of horizon chunk l (the 64-lane chunk geometry) and the last lane adds
  // the final cost: the same summation order as the persistent solver (ipm_persistent.hip), so
  // both drivers take identical accept / reject decisions
  double csum = 0.0;
  int ok = 1;
  const Chunks ch(N, 64);
  for (int k = ch.start(lane); k < ch.start(lane) + ch.len(lane); ++k) {
    double xt[NX], ut[NU];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)k * NX + i] + DX[(size_t)k * NX + i];
    NOC_UNROLL for (int j = 0; j < NU; ++j) ut[j] = U[(size_t)k * NU + j] + DU[(size_t)k * NU + j];
    ok &= f.feasible(xt, ut) ? 1 : 0;
    csum += f.stage_cost(xt, ut, bp);
  }
  if (lane == 63) {
    double xt[NX];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)N * NX + i] + DX[(size_t)N * NX + i];
    csum += f.final_cost(xt);
  }
  csum = wave_sum(csum);
  const bool traj_ok = __all(ok);
  // new_cost = where(feasible, total_cost(trial), inf)   (P:159-163, S:126-129)
  const double new_cost = traj_ok ? csum : INFINITY;
  // the accept rule and barrier schedule of every solver (ipm_schedule.h); no solve cap here, so
  // the retry accounting has the whole retry loop for room
  IpmState s;
  s.load(w, b);
  const AcceptOutcome o = accept_step(s, mode, new_cost, w.pred[b], w.feasible[b] != 0, w.flags, 501);
  if (o.take) {  // x <- x + dx, u <- u + du
    double* Xw = w.x + (size_t)b * (N + 1) * NX;
    double* Uw = w.u + (size_t)b * N * NU;
    for (int k = lane; k <= N; k += 64) {
      NOC_UNROLL for (int i = 0; i < NX; ++i) Xw[(size_t)k * NX + i] += DX[(size_t)k * NX + i];
      if (k < N) NOC_UNROLL for (int j = 0; j < NU; ++j) Uw[(size_t)k * NU + j] += DU[(size_t)k * NU + j];
    }
  }
  if (lane != 0) return;
  if (w.repeats) w.repeats[b] += o.rep;
  w.kkt_solves[b] = s.solves;
  w.inner[b] = s.inner;
  w.it[b] = s.it;
  w.rp[b] = s.rp;
  w.rinc[b] = s.rinc;
  if (o.stage_done) {
    w.total_it[b] = s.total_it;
    w.bp[b] = s.bp;
  }
  // the rollout of a new stage happens in the next step (ROLLOUT_PENDING, see rollout_kernel)
  int phase = resume_point(o.stage_done, o.relinearize, s.bp, w.flags);
  if (phase == NOC_PHASE_ROLLOUT) phase = NOC_PHASE_ROLLOUT_PENDING;
  if (phase == NOC_PHASE_SOLVE) w.reg[b] = candidate_reg(mode, s.rp, s.gnorm);
  w.phase[b] = phase;
