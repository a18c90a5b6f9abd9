// Body of linearize_kernel and its per-trajectory-parameter twin (ipm_kernels.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = w.N, L = w.lanes;
  const Chunks ch(N, L);
  if (t >= (long long)w.Bt * ch.cmax * L) return;
  const int b = (int)(t / ((long long)ch.cmax * L));
  const int rem = (int)(t % ((long long)ch.cmax * L));
  const int j = rem / L, l = rem % L;
  if (j >= ch.len(l) || w.phase[b] != NOC_PHASE_LINEARIZE) return;
  const int k = ch.start(l) + j;
  const size_t tn = (size_t)b * N + k;
  Fam<KIND, NX, NU> f(prm);
  const double bp = w.bp[b];
  double x[NX], u[NU];
  gload<NX>(w.x + ((size_t)b * (N + 1) + k) * NX, x);
  NOC_UNROLL for (int i = 0; i < NU; ++i) u[i] = w.u[tn * NU + i];
  double fx[NX * NX], fu[NX * NU], cx[NX], cu[NU];  // all stored tiled
  f.jac(x, u, fx, fu);
  f.stage_grad(x, u, bp, cx, cu);
  if constexpr (COMPACT) {
    using BS = BlockStruct<KIND, NX, NU, true>;
    constexpr int VA = BS::template nv<BF_A>(), VB = BS::template nv<BF_B>();
    double va[VA > 0 ? VA : 1], vb[VB > 0 ? VB : 1];
    BS::template compress<BF_A>(fx, va);
    BS::template compress<BF_B>(fu, vb);
    if constexpr (VA > 0) tstore_rt<VA>(w.A, L, ch.cmax, b, j, l, va);
    if constexpr (VB > 0) tstore_rt<VB>(w.B, L, ch.cmax, b, j, l, vb);
  } else {
    tstore_rt<NX * NX>(w.A, L, ch.cmax, b, j, l, fx);
    tstore_rt<NX * NU>(w.B, L, ch.cmax, b, j, l, fu);
  }
  tstore_rt<NX>(w.cx, L, ch.cmax, b, j, l, cx);
  tstore_rt<NU>(w.cu, L, ch.cmax, b, j, l, cu);
  const double lc = f.stage_cost(x, u, bp);
  tstore_rt<1>(w.lc, L, ch.cmax, b, j, l, &lc);
