// Body of derivatives_kernel and its per-trajectory-parameter twin (derivatives.hip), included
// inside both kernels: the text between the braces, moved here unchanged, so that both compile the
// same statements on their own by-value arguments (template parameters and arguments of the
// including kernel in scope).  Not a stand-alone header (no include guard on purpose).
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)a.B * a.N) return;
  const int N = a.N;
  const long long b = t / N;
  const size_t bk = (size_t)t;  // b * N + k
  const int k = (int)(t - b * N);
  Fam<KIND, NX, NU> f(prm);
  double x[NX], u[NU];
  NOC_UNROLL for (int i = 0; i < NX; ++i) x[i] = a.x[((size_t)b * (N + 1) + k) * NX + i];
  NOC_UNROLL for (int j = 0; j < NU; ++j) u[j] = a.u[bk * NU + j];
  const double bp = a.bp[b];
  double cx[NX], cu[NU];
  f.stage_grad(x, u, bp, cx, cu);
  NOC_UNROLL for (int i = 0; i < NX; ++i) a.cx[bk * NX + i] = cx[i];
  NOC_UNROLL for (int j = 0; j < NU; ++j) a.cu[bk * NU + j] = cu[j];
  // cxx, cuu, cxu: the stage cost's Hessian (ipm_family.h: stage_hess; for the quadratic-plus-
  // log-barrier cost of PR:40-50 / CR:36-45 diag(wx), diag(wu + barrier), 0 -- the wrapped
  // coordinate's mod has derivative 1)
  {
    double cxx[NX * NX], cuu[NU * NU], cxu[NX * NU];
    f.stage_hess(x, u, bp, cxx, cuu, cxu);
    NOC_UNROLL for (int i = 0; i < NX * NX; ++i) a.cxx[bk * NX * NX + i] = cxx[i];
    NOC_UNROLL for (int i = 0; i < NU * NU; ++i) a.cuu[bk * NU * NU + i] = cuu[i];
    NOC_UNROLL for (int i = 0; i < NX * NU; ++i) a.cxu[bk * NX * NU + i] = cxu[i];
  }
  double fx[NX * NX], fu[NX * NU];
  f.jac(x, u, fx, fu);
  NOC_UNROLL for (int i = 0; i < NX * NX; ++i) a.fx[bk * NX * NX + i] = fx[i];
  NOC_UNROLL for (int i = 0; i < NX * NU; ++i) a.fu[bk * NX * NU + i] = fu[i];
  // fxx[i] = d2 f_i / dx dx etc. (jacrev(jacrev(dynamics)) shapes (nx, nx, nx), (nx, nu, nu),
  // (nx, nx, nu)): the lambda-contracted Hessian at lambda = e_i
  NOC_UNROLL for (int i = 0; i < NX; ++i) {
    double l[NX], Hxx[NX * NX], Huu[NU * NU], Hxu[NX * NU];
    NOC_UNROLL for (int m = 0; m < NX; ++m) l[m] = (m == i) ? 1.0 : 0.0;
    NOC_UNROLL for (int m = 0; m < NX * NX; ++m) Hxx[m] = 0.0;
    NOC_UNROLL for (int m = 0; m < NU * NU; ++m) Huu[m] = 0.0;
    NOC_UNROLL for (int m = 0; m < NX * NU; ++m) Hxu[m] = 0.0;
    f.add_hess_l(x, u, l, Hxx, Huu, Hxu);
    NOC_UNROLL for (int m = 0; m < NX * NX; ++m) a.fxx[(bk * NX + i) * NX * NX + m] = Hxx[m];
    NOC_UNROLL for (int m = 0; m < NU * NU; ++m) a.fuu[(bk * NX + i) * NU * NU + m] = Huu[m];
    NOC_UNROLL for (int m = 0; m < NX * NU; ++m) a.fxu[(bk * NX + i) * NX * NU + m] = Hxu[m];
  }
