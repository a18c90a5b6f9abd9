// Body of assemble_kernel and its per-trajectory-parameter twin (ipm_kernels.hip), included
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
  double x[NX], u[NU], lam[NX];
  gload<NX>(w.x + ((size_t)b * (N + 1) + k) * NX, x);
  NOC_UNROLL for (int i = 0; i < NU; ++i) u[i] = w.u[tn * NU + i];
  gload<NX>(w.lam + ((size_t)b * (N + 1) + k + 1) * NX, lam);
  // Q = cxx + l.fxx ; R = cuu + l.fuu ; M = cxu + l.fxu  (P:35-37), l = lambda_{k+1}
  double Q[NX * NX], R[NU * NU], M[NX * NU];
  f.stage_hess(x, u, bp, Q, R, M);
  f.add_hess_l(x, u, lam, Q, R, M);
  Sym<NX> Qs;
  Sym<NU> Rs;
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    NOC_UNROLL for (int jj = i; jj < NX; ++jj) Qs(i, jj) = (i == jj) ? Q[i * NX + i] : 0.5 * (Q[i * NX + jj] + Q[jj * NX + i]);
  NOC_UNROLL for (int i = 0; i < NU; ++i)
    NOC_UNROLL for (int jj = i; jj < NU; ++jj) Rs(i, jj) = (i == jj) ? R[i * NU + i] : 0.5 * (R[i * NU + jj] + R[jj * NU + i]);
  if constexpr (COMPACT) {
    using BS = BlockStruct<KIND, NX, NU, true>;
    constexpr int VQ = BS::template nv<BF_Q>(), VR = BS::template nv<BF_R>(), VM = BS::template nv<BF_M>();
    double vq[VQ > 0 ? VQ : 1], vr[VR > 0 ? VR : 1], vm[VM > 0 ? VM : 1];
    BS::template compress<BF_Q>(Qs.v, vq);
    BS::template compress<BF_R>(Rs.v, vr);
    BS::template compress<BF_M>(M, vm);
    if constexpr (VQ > 0) tstore_rt<VQ>(w.Q, L, ch.cmax, b, j, l, vq);
    if constexpr (VR > 0) tstore_rt<VR>(w.R, L, ch.cmax, b, j, l, vr);
    if constexpr (VM > 0) tstore_rt<VM>(w.M, L, ch.cmax, b, j, l, vm);
  } else {
    tstore_rt<Sym<NX>::SZ>(w.Q, L, ch.cmax, b, j, l, Qs.v);
    tstore_rt<Sym<NU>::SZ>(w.R, L, ch.cmax, b, j, l, Rs.v);
    tstore_rt<NX * NU>(w.M, L, ch.cmax, b, j, l, M);
  }
  if (terminal == NOC_TERMINAL_STAGE0 && k == 0) gstore<NX * NX>(w.P + (size_t)b * NX * NX, Q);  // P:73
