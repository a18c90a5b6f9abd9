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
  const double cost = w.cost[b];
  const double pred = w.pred[b];
  const bool bwd_ok = w.feasible[b] != 0;
  const double gain = (new_cost - cost) / pred;           // P:164-165
  const bool success = (gain > 0.0) && bwd_ok;            // P:166 / S:137
  double rp = w.rp[b], rinc = w.rinc[b];
  const double rp_used = rp;
  const double shrink = rp_shrink(gain);  // P:169 / S:141 (noc_internal.h)
  rp = success ? rp * shrink : rp * rinc;                 // P:167-171 / S:139-143
  rinc = success ? 2.0 : 2.0 * rinc;                      // P:172 / S:144
  bool take, end_iter, stop;
  int inner = w.inner[b] + 1, rep = 0;
  if (mode == NOC_MODE_PAR) {
    rp = fmin(fmax(rp, 1e-16), 1e16);                     // P:173
    // identical retries at the rp clip: accounted, not recomputed (noc_internal.h)
    rep = par_retry_repeats(w, success, rp_used, rp, inner, 501);
    inner += rep;
    rinc = ldexp(rinc, rep);                              // r_inc doubles per retry (P:172)
    end_iter = success || inner > 500;                    // P:177-182
    take = end_iter;                                      // the last trial is kept (P:175, P:184)
    stop = end_iter && (w.hu[b] < 1e-4 || w.it[b] + 1 > 1000);  // P:199-202
  } else {
    take = success;                                       // S:145-146
    end_iter = true;
    stop = (w.hu[b] < 1e-4) && bwd_ok;                    // S:157-161
  }
  if (take) {  // x <- x + dx, u <- u + du
    double* Xw = w.x + (size_t)b * (N + 1) * NX;
    double* Uw = w.u + (size_t)b * N * NU;
    for (int k = lane; k <= N; k += 64) {
      NOC_UNROLL for (int i = 0; i < NX; ++i) Xw[(size_t)k * NX + i] += DX[(size_t)k * NX + i];
      if (k < N) NOC_UNROLL for (int j = 0; j < NU; ++j) Uw[(size_t)k * NU + j] += DU[(size_t)k * NU + j];
    }
  }
  if (lane != 0) return;
  w.kkt_solves[b] += 1 + rep;
  if (w.repeats) w.repeats[b] += rep;
  w.inner[b] = inner;
  int it = w.it[b] + (end_iter ? 1 : 0);
  int phase;
  if (stop) {                                             // barrier stage finished
    w.total_it[b] += it;                                  // P:239 / S:187
    const double nbp = bp / 5.0;                          // P:238 / S:186
    w.bp[b] = nbp;
    it = 0;
    rp = 1.0;                                             // P:134 / S:110
    rinc = 2.0;                                           // P:135 / S:111
    // P:243-245; the rollout of the new stage happens in the next step (ROLLOUT_PENDING, see
    // rollout_kernel)
    // (NOC_WS_ONE_STAGE: newton_oc runs a single barrier stage)
    phase = (nbp > 1e-4 && !(w.flags & NOC_WS_ONE_STAGE)) ? NOC_PHASE_ROLLOUT_PENDING : NOC_PHASE_DONE;
  } else if (mode == NOC_MODE_PAR) {
    phase = end_iter ? NOC_PHASE_LINEARIZE : NOC_PHASE_SOLVE;
  } else {
    // seq: the next iteration linearises at x (+step if taken); a rejected step leaves x, u
    // unchanged, so only the regularisation changes (same blocks, cheaper: skip relinearising)
    phase = success ? NOC_PHASE_LINEARIZE : NOC_PHASE_SOLVE;
  }
  w.it[b] = it;
  w.rp[b] = rp;
  w.rinc[b] = rinc;
  if (phase == NOC_PHASE_SOLVE) w.reg[b] = (mode == NOC_MODE_PAR) ? rp * w.gnorm[b] : rp;
  w.phase[b] = phase;
