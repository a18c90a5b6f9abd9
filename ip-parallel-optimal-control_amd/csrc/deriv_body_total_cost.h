// Body of total_cost_kernel and its per-trajectory-parameter twin (derivatives.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const int b = blockIdx.x;
  if (b >= B) return;
  Fam<KIND, NX, NU> f(prm);
  const double bpb = bp[b];
  double s = 0.0;
  for (int k = threadIdx.x; k < N; k += 64) {
    double xk[NX], uk[NU];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xk[i] = x[((size_t)b * (N + 1) + k) * NX + i];
    NOC_UNROLL for (int j = 0; j < NU; ++j) uk[j] = u[((size_t)b * N + k) * NU + j];
    s += f.stage_cost(xk, uk, bpb);
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    double xN[NX];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xN[i] = x[((size_t)b * (N + 1) + N) * NX + i];
    cost[b] = f.final_cost(xN) + s;
  }
