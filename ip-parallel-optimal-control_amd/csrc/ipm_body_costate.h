// Body of costate_scan_kernel and its per-trajectory-parameter twin (ipm_kernels.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid / L, l = tid % L;
  if (b >= w.Bt || !builds_blocks(w, b)) return;  // uniform per segment
  // a retry handed over by a persistent launch (ipm_schedule.h: blocks_missing): lam, r, P and
  // reg are rebuilt, the iteration's cost, |Hu|, ||cu|| and retry count stay as that launch left them
  const bool handed_over = w.phase[b] == NOC_PHASE_SOLVE;
  Fam<KIND, NX, NU> f(prm);
  const int N = w.N;
  const Chunks ch(N, L);
  const int start = ch.start(l), len = ch.len(l);
  const bool last = (l == L - 1);
  const double* xN = w.x + ((size_t)b * (N + 1) + N) * NX;
  double lamN[NX];
  f.final_grad(xN, lamN);  // grad(final_cost) (C:35)
  // a stage's A / B from the workspace (COMPACT: the stored variable entries + the constants)
  auto load_A = [&](int jj, double* A) {
    if constexpr (COMPACT) {
      using BS = BlockStruct<KIND, NX, NU, true>;
      constexpr int VA = BS::template nv<BF_A>();
      double va[VA > 0 ? VA : 1];
      if constexpr (VA > 0) tload_rt<VA>(w.A, L, ch.cmax, b, jj, l, va);
      BS::template expand<BF_A>(prm, va, A);
    } else {
      tload_rt<NX * NX>(w.A, L, ch.cmax, b, jj, l, A);
    }
  };
  auto load_B = [&](int jj, double* Bm) {
    if constexpr (COMPACT) {
      using BS = BlockStruct<KIND, NX, NU, true>;
      constexpr int VB = BS::template nv<BF_B>();
      double vb[VB > 0 ? VB : 1];
      if constexpr (VB > 0) tload_rt<VB>(w.B, L, ch.cmax, b, jj, l, vb);
      BS::template expand<BF_B>(prm, vb, Bm);
    } else {
      tload_rt<NX * NU>(w.B, L, ch.cmax, b, jj, l, Bm);
    }
  };
  // phases 1-2 (L > 1): chunk maps and their scan; L = 1 (grouped layout, one lane per
  // trajectory) sweeps the whole horizon from lambda_N directly
  Mat<NX, NX> G;
  Vec<NX> g;
  set_zero(g);
  if constexpr (L > 1) {
    // phase 1: chunk map lambda_start = G lambda_end + g
    set_identity(G);
    for (int k = start + len - 1; k >= start; --k) {
      double A[NX * NX], cx[NX];
      load_A(k - start, A);
      tload_rt<NX>(w.cx, L, ch.cmax, b, k - start, l, cx);
      Mat<NX, NX> Gn;
      Vec<NX> gn;
      NOC_UNROLL for (int i = 0; i < NX; ++i) {
        double t = cx[i];
        NOC_UNROLL for (int m = 0; m < NX; ++m) t += A[m * NX + i] * g[m];
        gn[i] = t;
        NOC_UNROLL for (int j = 0; j < NX; ++j) {
          double u = 0.0;
          NOC_UNROLL for (int m = 0; m < NX; ++m) u += A[m * NX + i] * G(m, j);
          Gn(i, j) = u;
        }
      }
      G = Gn;
      g = gn;
    }
    if (last) {  // the last chunk ends at the terminal costate: its map becomes constant
      NOC_UNROLL for (int i = 0; i < NX; ++i) {
        double t = g[i];
        NOC_UNROLL for (int m = 0; m < NX; ++m) t += G(i, m) * lamN[m];
        g[i] = t;
      }
      set_zero(G);
    }
    // phase 2: reverse Hillis-Steele; lanes without a partner get their own (already constant) map
  #pragma unroll 1
    for (int d = 1; d < L; d <<= 1) {
      Mat<NX, NX> G2;
      Vec<NX> g2;
      shfl_down_arr<NX * NX>(G.v, G2.v, d, L);
      shfl_down_arr<NX>(g.v, g2.v, d, L);
      Mat<NX, NX> Gn;
      NOC_UNROLL for (int i = 0; i < NX; ++i) {
        double t = g[i];
        NOC_UNROLL for (int m = 0; m < NX; ++m) t += G(i, m) * g2[m];
        g[i] = t;
        NOC_UNROLL for (int j = 0; j < NX; ++j) {
          double u = 0.0;
          NOC_UNROLL for (int m = 0; m < NX; ++m) u += G(i, m) * G2(m, j);
          Gn(i, j) = u;
        }
      }
      G = Gn;
    }
  }
  // phase 3: sweep the chunk from its true end costate
  double lam[NX];
  if constexpr (L > 1) shfl_down_arr<NX>(g.v, lam, 1, L);
  if (last) NOC_UNROLL for (int i = 0; i < NX; ++i) lam[i] = lamN[i];
  double* LAM = w.lam + (size_t)b * (N + 1) * NX;
  if (last) gstore<NX>(LAM + (size_t)N * NX, lamN);
  double cost = 0.0, hu = 0.0, g2s = 0.0;
  for (int k = start + len - 1; k >= start; --k) {
    double A[NX * NX], Bm[NX * NU], cx[NX], cu[NU], lc, rr[NU];
    load_A(k - start, A);
    load_B(k - start, Bm);
    tload_rt<NX>(w.cx, L, ch.cmax, b, k - start, l, cx);
    tload_rt<NU>(w.cu, L, ch.cmax, b, k - start, l, cu);
    tload_rt<1>(w.lc, L, ch.cmax, b, k - start, l, &lc);
    NOC_UNROLL for (int jj = 0; jj < NU; ++jj) {  // ru_k = cu_k + fu_k' lambda_{k+1}  (P:34)
      double r = cu[jj];
      NOC_UNROLL for (int i = 0; i < NX; ++i) r += Bm[i * NU + jj] * lam[i];
      rr[jj] = r;
      hu = nan_max(hu, fabs(r));
      g2s += cu[jj] * cu[jj];
    }
    tstore_rt<NU>(w.r, L, ch.cmax, b, k - start, l, rr);
    double ln[NX];
    NOC_UNROLL for (int i = 0; i < NX; ++i) {
      double t = cx[i];
      NOC_UNROLL for (int m = 0; m < NX; ++m) t += A[m * NX + i] * lam[m];
      ln[i] = t;
    }
    NOC_UNROLL for (int i = 0; i < NX; ++i) lam[i] = ln[i];
    gstore<NX>(LAM + (size_t)k * NX, lam);
    cost += lc;
  }
  // lambda at the chunk start := the scan's value g (not this lane's sweep): it is exactly the
  // boundary costate the previous lane used, so every consumer of lambda_k sees one value
  if (L > 1 && len > 0) gstore<NX>(LAM + (size_t)start * NX, g.v);
  NOC_UNROLL for (int off = L / 2; off > 0; off >>= 1) {
    cost += __shfl_xor(cost, off, L);
    g2s += __shfl_xor(g2s, off, L);
    hu = nan_max(hu, __shfl_xor(hu, off, L));
  }
  if (l != 0) return;
  double P[NX * NX];
  f.final_hess(xN, P);  // hessian(final_cost) (S:66)
  gstore<NX * NX>(w.P + (size_t)b * NX * NX, P);
  if (handed_over) {
    w.reg[b] = candidate_reg(mode, w.rp[b], w.gnorm[b]);
    return;
  }
  w.cost[b] = cost + f.final_cost(xN);   // total_cost(x, u, bp) (P:142)
  w.hu[b] = hu;                          // max |Hu| (P:158)
  const double gn = sqrt(g2s);           // ||cu||_F (P:116)
  w.gnorm[b] = gn;
  w.reg[b] = candidate_reg(mode, w.rp[b], gn);  // fed to the KKT solve (ipm_schedule.h)
  w.inner[b] = 0;
