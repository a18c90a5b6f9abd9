// The classical fourth-order Runge-Kutta stage map of an ODE (noc/utils.py:13-23, one step per
// stage) with its exact first and second derivatives, composed from the three generated functions
// of the ODE's right-hand side f: its value, its Jacobian J = d f / d[x; u] and its
// lambda-contracted Hessian (noc/_codegen.py).  Fam (ipm_family.h) calls it for a registered
// family with gen::kCustomIntegrator == kIntegratorRk4, so every solver gets it.
//
//   x+ = x + sum_i b_i k_i,   k_i = f(x_i, u),   x_i = x + a_i k_{i-1},
//   a = (0, h/2, h/2, h),     b = (h/6, h/3, h/3, h/6).
//
// With z_i = (x_i, u) and Z_i = d z_i / d z = [[T_i], [0 I]], T_i = [I 0] + a_i G_{i-1} (NX x NZ),
// G_i = d k_i / d z = J(z_i) Z_i = J_x(z_i) T_i + [0 J_u(z_i)]:
//   [fx | fu] = [I 0] + sum_i b_i G_i,
//   sum_j lam_j d2 x+_j = sum_i Z_i^T [ sum_j mu_i,j d2 f_j (z_i) ] Z_i,
// where mu_i is the adjoint of k_i: mu_4 = b_4 lam, mu_i = b_i lam + a_{i+1} J_x(z_{i+1})^T
// mu_{i+1} (lam . x+ is linear in every k_i, and k_{i+1} depends on k_i through x_{i+1} alone, so
// the second-order terms are exactly those of the four evaluations of f).  The step h is inside
// a and b: no factor outside.
//
// ODE is any type with the static members rhs(x, u, f), rhs_jac(x, u, J) (row-major NX x NZ) and
// rhs_hess_l(x, u, l, H) (row-major NZ x NZ).  Everything is per lane on fixed-size arrays with
// fully unrolled loops (NZ <= 12), so the arrays are registers (or scratch where the compiler runs
// out of them).  Needs NOC_DEV (small_linalg.h; a host build defines it as `static inline`).
#pragma once

#ifndef NOC_UNROLL
#define NOC_UNROLL
#endif

namespace noc {
namespace rk4 {

// x_i = x + a k
template <int NX>
NOC_DEV void stage_state(const double* x, double a, const double* k, double* xi) {
  NOC_UNROLL for (int i = 0; i < NX; ++i) xi[i] = x[i] + a * k[i];
}

template <class ODE, int NX, int NU>
NOC_DEV void step(double h, const double* x, const double* u, double* xn) {
  double k1[NX], k2[NX], k3[NX], k4[NX], xi[NX];
  ODE::rhs(x, u, k1);
  stage_state<NX>(x, 0.5 * h, k1, xi);
  ODE::rhs(xi, u, k2);
  stage_state<NX>(x, 0.5 * h, k2, xi);
  ODE::rhs(xi, u, k3);
  stage_state<NX>(x, h, k3, xi);
  ODE::rhs(xi, u, k4);
  // noc/utils.py:24
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    xn[i] = x[i] + h / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
}

// T = [I 0] + a G (the x rows of Z; G = d k_{i-1} / d z)
template <int NX, int NU>
NOC_DEV void stage_T(double a, const double* G, double* T) {
  constexpr int NZ = NX + NU;
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    NOC_UNROLL for (int j = 0; j < NZ; ++j) T[i * NZ + j] = (i == j ? 1.0 : 0.0) + a * G[i * NZ + j];
}
// G = J_x T + [0 J_u]
template <int NX, int NU>
NOC_DEV void stage_G(const double* J, const double* T, double* G) {
  constexpr int NZ = NX + NU;
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    NOC_UNROLL for (int j = 0; j < NZ; ++j) {
      double s = (j >= NX) ? J[i * NZ + j] : 0.0;
      NOC_UNROLL for (int k = 0; k < NX; ++k) s += J[i * NZ + k] * T[k * NZ + j];
      G[i * NZ + j] = s;
    }
}

// One stage of the first-order sweep at x_i = x + a k: k <- f(z_i), G <- d k / d z (from the
// previous stage's G), S += b G.  The first stage (a = 0) has T = [I 0]: G = J.
template <class ODE, int NX, int NU, bool FIRST>
NOC_DEV void jac_stage(double a, double b, const double* x, const double* u, double* k, double* G,
                       double* S) {
  constexpr int NZ = NX + NU;
  if constexpr (FIRST) {
    ODE::rhs(x, u, k);
    ODE::rhs_jac(x, u, G);
  } else {
    double xi[NX], T[NX * NZ], J[NX * NZ];
    stage_state<NX>(x, a, k, xi);
    stage_T<NX, NU>(a, G, T);
    ODE::rhs(xi, u, k);
    ODE::rhs_jac(xi, u, J);
    stage_G<NX, NU>(J, T, G);
  }
  NOC_UNROLL for (int e = 0; e < NX * NZ; ++e) S[e] += b * G[e];
}

template <class ODE, int NX, int NU>
NOC_DEV void jac(double h, const double* x, const double* u, double* fx, double* fu) {
  constexpr int NZ = NX + NU;
  double k[NX], G[NX * NZ], S[NX * NZ];
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    NOC_UNROLL for (int j = 0; j < NZ; ++j) S[i * NZ + j] = (i == j) ? 1.0 : 0.0;
  jac_stage<ODE, NX, NU, true>(0.0, h / 6.0, x, u, k, G, S);
  jac_stage<ODE, NX, NU, false>(0.5 * h, h / 3.0, x, u, k, G, S);
  jac_stage<ODE, NX, NU, false>(0.5 * h, h / 3.0, x, u, k, G, S);
  // the last stage's k is not needed: only its Jacobian
  jac_stage<ODE, NX, NU, false>(h, h / 6.0, x, u, k, G, S);
  NOC_UNROLL for (int i = 0; i < NX; ++i) {
    NOC_UNROLL for (int j = 0; j < NX; ++j) fx[i * NX + j] = S[i * NZ + j];
    NOC_UNROLL for (int j = 0; j < NU; ++j) fu[i * NU + j] = S[i * NZ + NX + j];
  }
}

// mu_prev = b lam + a J_x(z_i)^T mu
template <class ODE, int NX, int NU>
NOC_DEV void adjoint_stage(double a, double b, const double* xi, const double* u,
                           const double* lam, const double* mu, double* mu_prev) {
  constexpr int NZ = NX + NU;
  double J[NX * NZ];
  ODE::rhs_jac(xi, u, J);
  NOC_UNROLL for (int j = 0; j < NX; ++j) {
    double s = 0.0;
    NOC_UNROLL for (int i = 0; i < NX; ++i) s += J[i * NZ + j] * mu[i];
    mu_prev[j] = b * lam[j] + a * s;
  }
}

// Hxx, Hxu, Huu += the blocks of Z^T H(z_i, mu) Z with Z = [[T], [0 I]]
template <class ODE, int NX, int NU, bool FIRST>
NOC_DEV void hess_stage(const double* xi, const double* u, const double* mu, const double* T,
                        double* Hxx, double* Huu, double* Hxu) {
  constexpr int NZ = NX + NU;
  double H[NZ * NZ];
  ODE::rhs_hess_l(xi, u, mu, H);
  if constexpr (FIRST) {  // Z = I
    NOC_UNROLL for (int i = 0; i < NX; ++i) {
      NOC_UNROLL for (int j = 0; j < NX; ++j) Hxx[i * NX + j] += H[i * NZ + j];
      NOC_UNROLL for (int j = 0; j < NU; ++j) Hxu[i * NU + j] += H[i * NZ + NX + j];
    }
    NOC_UNROLL for (int i = 0; i < NU; ++i)
      NOC_UNROLL for (int j = 0; j < NU; ++j) Huu[i * NU + j] += H[(NX + i) * NZ + NX + j];
  } else {
    double W[NZ * NZ];  // W = H Z
    NOC_UNROLL for (int a = 0; a < NZ; ++a)
      NOC_UNROLL for (int c = 0; c < NZ; ++c) {
        double s = (c >= NX) ? H[a * NZ + c] : 0.0;
        NOC_UNROLL for (int k = 0; k < NX; ++k) s += H[a * NZ + k] * T[k * NZ + c];
        W[a * NZ + c] = s;
      }
    // (Z^T W)[d][c] = sum_k T[k][d] W[k][c] (+ W[d][c] in the u rows); the u-x block is the
    // transpose of the x-u block and is not formed
    NOC_UNROLL for (int d = 0; d < NZ; ++d)
      NOC_UNROLL for (int c = (d < NX ? 0 : NX); c < NZ; ++c) {
        double s = (d >= NX) ? W[d * NZ + c] : 0.0;
        NOC_UNROLL for (int k = 0; k < NX; ++k) s += T[k * NZ + d] * W[k * NZ + c];
        if (d < NX && c < NX) Hxx[d * NX + c] += s;
        else if (d < NX) Hxu[d * NU + (c - NX)] += s;
        else Huu[(d - NX) * NU + (c - NX)] += s;
      }
  }
}

// sum_j lam_j d2 x+_j / dz dz added into Hxx (NX x NX), Huu (NU x NU), Hxu (NX x NU).  Three
// sweeps, so that no stage's NX x NZ sensitivity outlives its use: the stage states forward, the
// adjoints mu_i backward (Jacobians only), then forward again with T_i beside the contracted
// Hessian of one stage at a time.
template <class ODE, int NX, int NU>
NOC_DEV void add_hess_l(double h, const double* x, const double* u, const double* lam,
                        double* Hxx, double* Huu, double* Hxu) {
  constexpr int NZ = NX + NU;
  double x2[NX], x3[NX], x4[NX], k[NX];
  ODE::rhs(x, u, k);
  stage_state<NX>(x, 0.5 * h, k, x2);
  ODE::rhs(x2, u, k);
  stage_state<NX>(x, 0.5 * h, k, x3);
  ODE::rhs(x3, u, k);
  stage_state<NX>(x, h, k, x4);

  double mu1[NX], mu2[NX], mu3[NX], mu4[NX];
  NOC_UNROLL for (int i = 0; i < NX; ++i) mu4[i] = h / 6.0 * lam[i];
  adjoint_stage<ODE, NX, NU>(h, h / 3.0, x4, u, lam, mu4, mu3);
  adjoint_stage<ODE, NX, NU>(0.5 * h, h / 3.0, x3, u, lam, mu3, mu2);
  adjoint_stage<ODE, NX, NU>(0.5 * h, h / 6.0, x2, u, lam, mu2, mu1);

  double G[NX * NZ], T[NX * NZ], J[NX * NZ];
  hess_stage<ODE, NX, NU, true>(x, u, mu1, nullptr, Hxx, Huu, Hxu);
  ODE::rhs_jac(x, u, G);  // G_1 = J(z_1)
  stage_T<NX, NU>(0.5 * h, G, T);
  hess_stage<ODE, NX, NU, false>(x2, u, mu2, T, Hxx, Huu, Hxu);
  ODE::rhs_jac(x2, u, J);
  stage_G<NX, NU>(J, T, G);
  stage_T<NX, NU>(0.5 * h, G, T);
  hess_stage<ODE, NX, NU, false>(x3, u, mu3, T, Hxx, Huu, Hxu);
  ODE::rhs_jac(x3, u, J);
  stage_G<NX, NU>(J, T, G);
  stage_T<NX, NU>(h, G, T);
  hess_stage<ODE, NX, NU, false>(x4, u, mu4, T, Hxx, Huu, Hxu);
}

}  // namespace rk4
}  // namespace noc
