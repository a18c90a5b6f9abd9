// Body of final_derivs_kernel and its per-trajectory-parameter twin (derivatives.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Fam<KIND, NX, NU> f(prm);
  double x[NX];
  NOC_UNROLL for (int i = 0; i < NX; ++i) x[i] = xN[(size_t)b * NX + i];
  double g[NX];
  f.final_grad(x, g);
  NOC_UNROLL for (int i = 0; i < NX; ++i) grad[(size_t)b * NX + i] = g[i];
  if (hess) {
    double H[NX * NX];
    f.final_hess(x, H);
    NOC_UNROLL for (int i = 0; i < NX * NX; ++i) hess[(size_t)b * NX * NX + i] = H[i];
  }
