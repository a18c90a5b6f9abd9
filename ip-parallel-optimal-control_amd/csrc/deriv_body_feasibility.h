// Body of feasibility_kernel and its per-trajectory-parameter twin (derivatives.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const int b = blockIdx.x;
  if (b >= B) return;
  Fam<KIND, NX, NU> f(prm);
  bool good = true;
  for (int k = threadIdx.x; k < N; k += 64) {
    double xk[NX], uk[NU];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xk[i] = x[((size_t)b * (N + 1) + k) * NX + i];
    NOC_UNROLL for (int j = 0; j < NU; ++j) uk[j] = u[((size_t)b * N + k) * NU + j];
    good = good && f.feasible(xk, uk);
  }
  const bool all = __all(good);
  if (threadIdx.x == 0) ok[b] = all ? 1 : 0;
