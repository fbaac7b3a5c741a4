// The host mathematics behind every fast-diagonalisation preconditioner: the 1D FE_Q(k) mass / stiffness matrices of a grid line, their generalised eigenpairs with or
// without the end nodes, the even / odd classification of the eigenvectors, and the packing of transform matrices into MFMA fragment order.
// Plain host code without HIP types (compiles on its own); the kernel files upload what the packers return.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <stdexcept>
#include <vector>

namespace poro {
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };      // every failure of the back end; declared here because this header compiles alone

// symmetric eigenproblem by cyclic Jacobi rotations (n <= 320: a few 1e8 flop, once per mesh); V's columns are the eigenvectors
inline void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &V, std::vector<double> &w) {
  V.assign((size_t)n * n, 0.0); for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int i = 0; i < n; ++i) { diag += A[(size_t)i * n + i] * A[(size_t)i * n + i]; for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j]; }
    if (off <= 1e-30 * diag || off == 0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (std::fabs(apq) < 1e-300) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < n; ++k) {   // columns p, q
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = cs * akp - sn * akq; A[(size_t)k * n + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; ++k) {   // rows p, q
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = cs * apk - sn * aqk; A[(size_t)q * n + k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = cs * vkp - sn * vkq; V[(size_t)k * n + q] = sn * vkp + cs * vkq;
        }
      }
  }
  w.resize(n); for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}

// symmetric eigenproblem by Householder tridiagonalisation + implicit QL with accumulated transformations (the classical tred2 / tql2 pair):
// O(n^3) with a small constant, for the long lines (n = 671 in BASELINE config 2) where the Jacobi sweeps above would take minutes.
// A is overwritten; V's columns are the eigenvectors.
inline void householder_ql_eig(int n, std::vector<double> &A, std::vector<double> &V, std::vector<double> &w) {
  std::vector<double> d(n, 0.0), e(n, 0.0);
  auto a = [&](int i, int j) -> double & { return A[(size_t)i * n + j]; };
  for (int i = n - 1; i > 0; --i) {
    const int l = i - 1; double h = 0, scale = 0;
    if (l > 0) {
      for (int k = 0; k <= l; ++k) scale += std::fabs(a(i, k));
      if (scale == 0.0) e[i] = a(i, l);
      else {
        for (int k = 0; k <= l; ++k) { a(i, k) /= scale; h += a(i, k) * a(i, k); }
        double f = a(i, l), g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
        e[i] = scale * g; h -= f * g; a(i, l) = f - g; f = 0.0;
        for (int j = 0; j <= l; ++j) {
          a(j, i) = a(i, j) / h;
          g = 0.0;
          for (int k = 0; k <= j; ++k) g += a(j, k) * a(i, k);
          for (int k = j + 1; k <= l; ++k) g += a(k, j) * a(i, k);
          e[j] = g / h; f += e[j] * a(i, j);
        }
        const double hh = f / (h + h);
        for (int j = 0; j <= l; ++j) {
          f = a(i, j); e[j] = g = e[j] - hh * f;
          for (int k = 0; k <= j; ++k) a(j, k) -= f * e[k] + g * a(i, k);
        }
      }
    } else e[i] = a(i, l);
    d[i] = h;
  }
  d[0] = 0.0; e[0] = 0.0;
  for (int i = 0; i < n; ++i) {
    const int l = i - 1;
    if (d[i] != 0.0)
      for (int j = 0; j <= l; ++j) {
        double g = 0.0;
        for (int k = 0; k <= l; ++k) g += a(i, k) * a(k, j);
        for (int k = 0; k <= l; ++k) a(k, j) -= g * a(k, i);
      }
    d[i] = a(i, i); a(i, i) = 1.0;
    for (int j = 0; j <= l; ++j) a(j, i) = a(i, j) = 0.0;
  }
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  for (int l = 0; l < n; ++l) {
    int iter = 0, m;
    do {
      for (m = l; m < n - 1; ++m) { const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]); if (std::fabs(e[m]) <= 1e-16 * dd) break; }
      if (m != l) {
        if (iter++ == 200) throw Error("householder_ql_eig: no convergence");
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]), r = std::hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
        double sn = 1.0, cs = 1.0, p = 0.0; int i;
        for (i = m - 1; i >= l; --i) {
          double f = sn * e[i]; const double b = cs * e[i];
          e[i + 1] = (r = std::hypot(f, g));
          if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }
          sn = f / r; cs = g / r; g = d[i + 1] - p;
          r = (d[i] - g) * sn + 2.0 * cs * b;
          d[i + 1] = g + (p = sn * r); g = cs * r - b;
          for (int k = 0; k < n; ++k) { f = a(k, i + 1); a(k, i + 1) = sn * a(k, i) + cs * f; a(k, i) = cs * a(k, i) - sn * f; }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p; e[l] = g; e[m] = 0.0;
      }
    } while (m != l);
  }
  V = A; w = d;
}

// largest eigenvalue of a small dense symmetric matrix
inline double sym_lambda_max(int n, const std::vector<double> &A) {
  std::vector<double> B = A, V, w; jacobi_eig(n, B, V, w);
  double m = 0; for (double v : w) m = std::max(m, v);
  return m;
}
// largest eigenvalue of D^-1/2 A D^-1/2 for a small dense symmetric matrix (row-major n x n), D = diag(A): the rigorous element-level bound
// lambda_max(D^-1 A_global) <= max_e lambda_max(diag(A_e)^-1 A_e) of the Chebyshev preconditioner
inline double jacobi_scaled_lambda_max(int n, const std::vector<double> &A) {
  std::vector<double> B((size_t)n * n), V, w;
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) B[(size_t)i * n + j] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]) / std::sqrt(A[(size_t)i * n + i] * A[(size_t)j * n + j]);
  jacobi_eig(n, B, V, w);
  double m = 0; for (double v : w) m = std::max(m, v);
  return m;
}

// The tables of one grid line.  S: n x n row-major, columns = M-orthonormal eigenvectors; lam: eigenvalues; parity: every mode is even or odd about the centre, listed in `even` / `odd`
struct LineTables { int n = 0; std::vector<double> S, lam; bool parity = false; std::vector<int> even, odd; };
// even / odd classification of the eigenvectors by their symmetry about the centre; removed modes (lam not finite) are skipped.  parity = false - "not split" - as
// soon as a mode is neither, or where a group comes out larger than the half line (n + 1) / 2 that the even / odd forms store
inline void classify_parity(LineTables &T) {
  const int n = T.n, h = (n + 1) / 2; const std::vector<double> &S = T.S;
  T.parity = true; T.even.clear(); T.odd.clear();
  for (int m = 0; m < n && T.parity; ++m) {
    if (!(T.lam[m] < 1e300)) continue;              // removed modes
    double ds = 0, da = 0, nrm = 0;
    for (int k = 0; k < n; ++k) { const double a = S[(size_t)k * n + m], b = S[(size_t)(n - 1 - k) * n + m]; ds += (a - b) * (a - b); da += (a + b) * (a + b); nrm += a * a; }
    if (ds <= 1e-20 * nrm) T.even.push_back(m); else if (da <= 1e-20 * nrm) T.odd.push_back(m); else T.parity = false;
  }
  T.parity = T.parity && (int)T.even.size() <= h && (int)T.odd.size() <= h;
  if (!T.parity) { T.even.clear(); T.odd.clear(); }
}
// FE_Q(k) mass / stiffness matrices of n_cells cells of length h (dense, nn = k n_cells + 1); element matrices as in kernels_kron.hip
inline void fe1d(int k, const std::vector<double> &hc, std::vector<double> &M, std::vector<double> &K) {
  const int n_cells = (int)hc.size(), nn = k * n_cells + 1; M.assign((size_t)nn * nn, 0.0); K.assign((size_t)nn * nn, 0.0);
  static const double M2[3][3] = {{4, 2, -1}, {2, 16, 2}, {-1, 2, 4}}, K2[3][3] = {{7, -8, 1}, {-8, 16, -8}, {1, -8, 7}};
  static const double M1[2][2] = {{2, 1}, {1, 2}}, K1[2][2] = {{1, -1}, {-1, 1}};
  for (int c = 0; c < n_cells; ++c)
    for (int a = 0; a <= k; ++a) for (int b = 0; b <= k; ++b) {
      const size_t at = (size_t)(k * c + a) * nn + (k * c + b);
      const double h = hc[c];
      if (k == 2) { M[at] += h / 30.0 * M2[a][b]; K[at] += K2[a][b] / (3.0 * h); } else { M[at] += h / 6.0 * M1[a][b]; K[at] += K1[a][b] / h; }
    }
}

// generalised eigenpairs K s = lam M s of the 1D FE_Q(k) matrices on cells of the sizes hc, with the end nodes lo / hi removed when fix_lo / fix_hi:
// S (nn x nn row-major, S^T M S = I on the free block, zero rows for removed nodes, zero columns behind the n_free modes), lam (inf behind n_free)
inline LineTables line_tables(int k, const std::vector<double> &hc, bool fix_lo, bool fix_hi) {
  const int n_cells = (int)hc.size();
  std::vector<double> M, K; fe1d(k, hc, M, K);
  const int nn = k * n_cells + 1, f0 = fix_lo ? 1 : 0, nf = nn - f0 - (fix_hi ? 1 : 0);
  LineTables T; T.n = nn; std::vector<double> &S = T.S, &lam = T.lam;
  S.assign((size_t)nn * nn, 0.0); lam.assign(nn, std::numeric_limits<double>::infinity());
  if (nf <= 0) return T;
  // Cholesky M_ff = L L^T, C = L^-1 K_ff L^-T, C = Q W Q^T, S_ff = L^-T Q
  std::vector<double> Lc((size_t)nf * nf, 0.0), C((size_t)nf * nf);
  for (int i = 0; i < nf; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = M[(size_t)(i + f0) * nn + (j + f0)];
      for (int p = 0; p < j; ++p) s -= Lc[(size_t)i * nf + p] * Lc[(size_t)j * nf + p];
      if (i == j) { if (!(s > 0)) throw Error("fdmu_eig_1d: mass matrix not positive definite"); Lc[(size_t)i * nf + i] = std::sqrt(s); }
      else Lc[(size_t)i * nf + j] = s / Lc[(size_t)j * nf + j];
    }
  // X = L^-1 K_ff (forward substitution on columns), C = X L^-T = (L^-1 X^T)^T
  std::vector<double> X((size_t)nf * nf);
  for (int col = 0; col < nf; ++col)
    for (int i = 0; i < nf; ++i) {
      double s = K[(size_t)(i + f0) * nn + (col + f0)];
      for (int p = 0; p < i; ++p) s -= Lc[(size_t)i * nf + p] * X[(size_t)p * nf + col];
      X[(size_t)i * nf + col] = s / Lc[(size_t)i * nf + i];
    }
  for (int row = 0; row < nf; ++row)         // solve L y = X[row, :]^T  ->  C[:, row] = y
    for (int i = 0; i < nf; ++i) {
      double s = X[(size_t)row * nf + i];
      for (int p = 0; p < i; ++p) s -= Lc[(size_t)i * nf + p] * C[(size_t)p * nf + row];
      C[(size_t)i * nf + row] = s / Lc[(size_t)i * nf + i];
    }
  for (int i = 0; i < nf; ++i) for (int j = i + 1; j < nf; ++j) { const double a = 0.5 * (C[(size_t)i * nf + j] + C[(size_t)j * nf + i]); C[(size_t)i * nf + j] = C[(size_t)j * nf + i] = a; }
  std::vector<double> Q, wv;
  if (nf > 96) householder_ql_eig(nf, C, Q, wv); else jacobi_eig(nf, C, Q, wv);
  for (int j = 0; j < nf; ++j) {             // back substitution L^T s = q_j
    std::vector<double> sv(nf);
    for (int i = nf - 1; i >= 0; --i) {
      double s = Q[(size_t)i * nf + j];
      for (int p = i + 1; p < nf; ++p) s -= Lc[(size_t)p * nf + i] * sv[p];
      sv[i] = s / Lc[(size_t)i * nf + i];
    }
    for (int i = 0; i < nf; ++i) S[(size_t)(i + f0) * nn + j] = sv[i];
    lam[j] = std::max(wv[j], 0.0);
  }
  // the same condition at both ends: M and K are persymmetric, every eigenvector is symmetric or antisymmetric about the centre up to the rounding of
  // the eigen-solver (1e-9 for the clustered top of a 671-point spectrum).  Make that exact - the even / odd transform kernels rely on it - and restore
  // the M-normalisation.
  if (fix_lo == fix_hi)
    for (int j = 0; j < nf; ++j) {
      double ds = 0, da = 0;
      for (int k = 0; k < nn; ++k) { const double a = S[(size_t)k * nn + j], b = S[(size_t)(nn - 1 - k) * nn + j]; ds += (a - b) * (a - b); da += (a + b) * (a + b); }
      const double sgn = ds <= da ? 1.0 : -1.0;
      if (std::min(ds, da) > 1e-8 * std::max(ds, da)) continue;         // (not the expected structure: left alone, the full-length kernels take over)
      for (int k = 0; k < nn / 2; ++k) {
        const double a = S[(size_t)k * nn + j], b = S[(size_t)(nn - 1 - k) * nn + j], v = 0.5 * (a + sgn * b);
        S[(size_t)k * nn + j] = v; S[(size_t)(nn - 1 - k) * nn + j] = sgn * v;
      }
      if ((nn & 1) && sgn < 0) S[(size_t)(nn / 2) * nn + j] = 0.0;
      double nrm = 0;
      for (int i = 0; i < nn; ++i) { double t = 0; for (int p = std::max(0, i - 2 * k); p <= std::min(nn - 1, i + 2 * k); ++p) t += M[(size_t)i * nn + p] * S[(size_t)p * nn + j]; nrm += S[(size_t)i * nn + j] * t; }
      const double sc = 1.0 / std::sqrt(nrm);
      for (int i = 0; i < nn; ++i) S[(size_t)i * nn + j] *= sc;
    }
  classify_parity(T);
  return T;
}

// K1 s = lam M1 s for the 1D Q1 matrices on n cells of size h (natural boundary conditions) in closed form:
// M1 = h/6 tridiag(1 4 1) (corners 2), K1 = 1/h tridiag(-1 2 -1) (corners 1): the eigenvectors are the cosines s_j(i) = cos(j pi i / n),
// lam_j = 6/h^2 (1 - cos t)/(2 + cos t), t = j pi / n (insert into an interior and a boundary row); columns scaled to s^T M1 s = 1.
inline LineTables q1_eig(int n_cells, double h) {
  const int n = n_cells + 1; const double pi = 3.14159265358979323846;
  LineTables T; T.n = n; std::vector<double> &S = T.S, &lam = T.lam;
  S.assign((size_t)n * n, 0.0); lam.assign(n, 0.0);
  std::vector<double> v(n);
  for (int j = 0; j < n; ++j) {
    const double t = j * pi / n_cells, ct = std::cos(t);
    lam[j] = 6.0 / (h * h) * (1.0 - ct) / (2.0 + ct);
    for (int i = 0; i < n; ++i) v[i] = std::cos(t * i);
    double m = 0;
    for (int i = 0; i < n; ++i) {
      double Mv = (i > 0 && i < n - 1 ? 4.0 : 2.0) * v[i];
      if (i > 0) Mv += v[i - 1];
      if (i < n - 1) Mv += v[i + 1];
      m += v[i] * Mv * h / 6.0;
    }
    const double sc = 1.0 / std::sqrt(m);
    for (int i = 0; i < n; ++i) S[(size_t)i * n + j] = v[i] * sc;
  }
  classify_parity(T);
  return T;
}

// MFMA fragment order, one lane map for every transform matrix: lane l of the fragment (tile, k-step) holds element (16 tile + (l & 15), 4 k-step + (l >> 4)).
// a rows x cols matrix el(r, c) as [tile][k-step][64], zero beyond rows / cols
template <class T, class El> std::vector<T> pack_fragments(int tiles, int ksteps, int rows, int cols, El el) {
  std::vector<T> f((size_t)tiles * ksteps * 64, (T)0);
  for (int t = 0; t < tiles; ++t) for (int kk = 0; kk < ksteps; ++kk) for (int l = 0; l < 64; ++l) {
    const int r = 16 * t + (l & 15), c = 4 * kk + (l >> 4);
    if (r < rows && c < cols) f[((size_t)t * ksteps + kk) * 64 + l] = (T)el(r, c);
  }
  return f;
}
// a whole line's transform in fragment order: forward F[mode][node] = S^T, backward B[node][mode] = S - every mode of the line; removed ones are zero columns of S
inline std::vector<double> whole_line_fragments(const LineTables &T, int tiles, bool backward) {
  const int n = T.n; const std::vector<double> &S = T.S;
  return backward ? pack_fragments<double>(tiles, 4 * tiles, n, n, [&](int r, int c) { return S[(size_t)r * n + c]; })
                  : pack_fragments<double>(tiles, 4 * tiles, n, n, [&](int r, int c) { return S[(size_t)c * n + r]; });
}

// ---- class-split form of a uniform Q2 line with equal ends ----
// On such a line the vertex nodes and the midpoint nodes each carry pure trigonometric vectors (free ends: cos(m pi i / (nn - 1)), removed ends: the sines): with
// a_m = that function on the vertices (zero on the midpoints) and b_m = the same on the midpoints, K and M couple a_m and b_m only with each other.  The M-orthonormal
// eigenvectors are therefore F = S W, S = blockdiag(S_v, S_m) after sorting the nodes by class and W one 2 x 2 generalised eigenvector matrix per frequency (1 x 1 where a
// class vanishes): a half-line transform becomes two class transforms of half the length plus two FMAs per entry.
// Per parity group (0: even modes, 1: odd): lower-half node 2 p is position p of the vertex class, node 2 p + 1 position p of the midpoint class (the centre node goes by
// its index); the frequencies of the group, ascending, are the slots 0, 1, ... of BOTH classes, and the two modes of a frequency take its slot in each class.
struct ClassSplitGroup {
  int nv = 0, nm = 0;                 // positions per class: (h + 1) / 2 and h / 2 of the h = (nn + 1) / 2 lower-half nodes
  int slots = 0;                      // frequencies of the group
  std::vector<double> Fv, Fm;         // class transforms [slot][position] (zero rows where the class has no vector at that frequency)
  std::vector<double> mix;            // [slot][4] = w_vv, w_mv, w_vm, w_mm: mode (v, s) = w_vv (Fv g_v)[s] + w_mv (Fm g_m)[s], mode (m, s) = w_vm (Fv g_v)[s] + w_mm (Fm g_m)[s]
  std::vector<double> lam_v, lam_m;   // [slot]: eigenvalues of the two modes (inf: no such mode)
};
struct ClassSplitTables {
  bool ok = false; const char *why = ""; int n = 0; ClassSplitGroup grp[2];
  double off_block = 0, orth = 0, resid = 0, eig_dev = 0;      // what the verification measured (relative figures)
};
// The verdict comes from the numbers: the trigonometric vectors are built from the node INDEX, the pencils from the line's own fe1d matrices, and the result is accepted only
// if (1) the off-block entries of S^T K S and S^T M S are <= 1e-12 of the largest entry, (2) F^T M F = I and F^T K F = Lambda to 1e-12 (the latter relative to the largest
// eigenvalue) and (3) the sorted eigenvalues equal those of T = line_tables(...) to 1e-12 of the largest.  A graded line fails (1); lines without classes (Q1), without
// parity (different ends) or of another length than T are turned down before.
inline ClassSplitTables class_split_tables(int k, const std::vector<double> &hc, bool fix_lo, bool fix_hi, const LineTables &T) {
  ClassSplitTables R; const int N = (int)hc.size(), nn = 2 * N + 1, h = (nn + 1) / 2; R.n = nn;
  if (k != 2) { R.why = "no midpoint class (not Q2)"; return R; }
  if (T.n != nn || !T.parity || fix_lo != fix_hi) { R.why = "modes without parity"; return R; }
  const bool fix = fix_lo; const double pi = 3.14159265358979323846, kTol = 1e-12;
  std::vector<double> M, K; fe1d(2, hc, M, K);
  auto band = [&](const std::vector<double> &A, const std::vector<double> &x, std::vector<double> &y) {
    y.assign(nn, 0.0);
    for (int i = 0; i < nn; ++i) for (int p = std::max(0, i - 2); p <= std::min(nn - 1, i + 2); ++p) y[i] += A[(size_t)i * nn + p] * x[p];
  };
  auto dot = [&](const std::vector<double> &x, const std::vector<double> &y) { double s = 0; for (int i = 0; i < nn; ++i) s += x[i] * y[i]; return s; };
  // class vectors of every frequency; a vector that vanishes (cosines on the midpoints at m = N, sines on the vertices at m = N) is absent
  struct Vec { int m, cls; std::vector<double> v, Mv, Kv; };
  std::vector<Vec> vecs; std::vector<int> at_v(N + 1, -1), at_m(N + 1, -1);
  for (int m = fix ? 1 : 0; m <= N; ++m) for (int cls = 0; cls < 2; ++cls) {
    Vec V; V.m = m; V.cls = cls; V.v.assign(nn, 0.0); double big = 0;
    for (int i = cls; i < nn; i += 2) { V.v[i] = (fix && (i == 0 || i == nn - 1)) ? 0.0 : fix ? std::sin(m * pi * i / (2.0 * N)) : std::cos(m * pi * i / (2.0 * N)); big = std::max(big, std::fabs(V.v[i])); }
    if (big < 1e-9) continue;
    band(M, V.v, V.Mv); band(K, V.v, V.Kv);
    (cls ? at_m : at_v)[m] = (int)vecs.size(); vecs.push_back(std::move(V));
  }
  const int nvec = (int)vecs.size();
  // (1) S^T K S and S^T M S: nothing outside the 2 x 2 blocks
  { double big = 0, off = 0;
    for (int w = 0; w < 2; ++w) {
      double bw = 0, ow = 0;
      for (int a = 0; a < nvec; ++a) for (int b = 0; b < nvec; ++b) {
        const double e = std::fabs(dot(vecs[a].v, w ? vecs[b].Mv : vecs[b].Kv));
        bw = std::max(bw, e); if (vecs[a].m != vecs[b].m) ow = std::max(ow, e);
      }
      big = std::max(big, bw); if (bw > 0) off = std::max(off, ow / bw);
    }
    R.off_block = off;
    if (!(big > 0) || !(off <= kTol)) { R.why = "vertex / midpoint classes couple across frequencies"; return R; } }
  // the pencils, frequency by frequency; full-line eigenvectors for the checks below
  for (int p = 0; p < 2; ++p) { R.grp[p].nv = (h + 1) / 2; R.grp[p].nm = h / 2; }
  std::vector<std::vector<double>> Fcol; std::vector<double> Flam; const double inf = std::numeric_limits<double>::infinity();
  for (int m = fix ? 1 : 0; m <= N; ++m) {
    const int ia = at_v[m], ib = at_m[m];
    if (ia < 0 && ib < 0) continue;
    const std::vector<double> &ref = vecs[ia >= 0 ? ia : ib].v;
    double ds = 0, da = 0;
    for (int i = 0; i < nn; ++i) { const double a = ref[i], b = ref[nn - 1 - i]; ds += (a - b) * (a - b); da += (a + b) * (a + b); }
    if (std::min(ds, da) > 1e-20 * std::max(ds, da)) { R.why = "a class vector is neither even nor odd"; return R; }
    ClassSplitGroup &G = R.grp[ds <= da ? 0 : 1]; const int s = G.slots++;
    G.Fv.resize((size_t)G.slots * G.nv, 0.0); G.Fm.resize((size_t)G.slots * G.nm, 0.0); G.mix.resize((size_t)G.slots * 4, 0.0); G.lam_v.resize(G.slots, inf); G.lam_m.resize(G.slots, inf);
    if (ia >= 0) for (int q = 0; q < G.nv; ++q) G.Fv[(size_t)s * G.nv + q] = vecs[ia].v[2 * q];
    if (ib >= 0) for (int q = 0; q < G.nm; ++q) G.Fm[(size_t)s * G.nm + q] = vecs[ib].v[2 * q + 1];
    double *w = &G.mix[(size_t)s * 4];
    if (ia >= 0 && ib >= 0) {
      const double maa = dot(vecs[ia].v, vecs[ia].Mv), mab = dot(vecs[ia].v, vecs[ib].Mv), mbb = dot(vecs[ib].v, vecs[ib].Mv);
      const double kr[2][2] = {{dot(vecs[ia].v, vecs[ia].Kv), dot(vecs[ia].v, vecs[ib].Kv)}, {dot(vecs[ib].v, vecs[ia].Kv), dot(vecs[ib].v, vecs[ib].Kv)}};
      if (!(maa > 0)) { R.why = "class mass block not positive definite"; return R; }
      const double l11 = std::sqrt(maa), l21 = mab / l11, d2 = mbb - l21 * l21;
      if (!(d2 > 0)) { R.why = "class mass block not positive definite"; return R; }
      const double l22 = std::sqrt(d2);
      // C = L^-1 Kr L^-T, C = Q diag(lam) Q^T, W = L^-T Q
      double X[2][2], Z[2][2];
      for (int j = 0; j < 2; ++j) { X[0][j] = kr[0][j] / l11; X[1][j] = (kr[1][j] - l21 * X[0][j]) / l22; }
      for (int j = 0; j < 2; ++j) { Z[0][j] = X[j][0] / l11; Z[1][j] = (X[j][1] - l21 * Z[0][j]) / l22; }      // Z = L^-1 X^T = C^T
      std::vector<double> C = {Z[0][0], 0.5 * (Z[0][1] + Z[1][0]), 0.5 * (Z[0][1] + Z[1][0]), Z[1][1]}, Q, lam;
      jacobi_eig(2, C, Q, lam);
      const int jv = lam[0] <= lam[1] ? 0 : 1, jm = 1 - jv;           // the lower mode of the pair takes the vertex slot
      const int js[2] = {jv, jm};
      for (int e = 0; e < 2; ++e) { const double q0 = Q[js[e]], q1 = Q[2 + js[e]], w1 = q1 / l22, w0 = (q0 - l21 * w1) / l11; w[2 * e] = w0; w[2 * e + 1] = w1; }
      G.lam_v[s] = std::max(lam[jv], 0.0); G.lam_m[s] = std::max(lam[jm], 0.0);
    } else if (ia >= 0) { const double maa = dot(vecs[ia].v, vecs[ia].Mv); w[0] = 1.0 / std::sqrt(maa); G.lam_v[s] = std::max(dot(vecs[ia].v, vecs[ia].Kv) / maa, 0.0); }
    else { const double mbb = dot(vecs[ib].v, vecs[ib].Mv); w[3] = 1.0 / std::sqrt(mbb); G.lam_m[s] = std::max(dot(vecs[ib].v, vecs[ib].Kv) / mbb, 0.0); }
    for (int e = 0; e < 2; ++e) {
      const double lam_e = e ? G.lam_m[s] : G.lam_v[s];
      if (!(lam_e < 1e300)) continue;
      std::vector<double> f(nn, 0.0);
      for (int i = 0; i < nn; ++i) f[i] = (ia >= 0 ? w[2 * e] * vecs[ia].v[i] : 0.0) + (ib >= 0 ? w[2 * e + 1] * vecs[ib].v[i] : 0.0);
      Fcol.push_back(std::move(f)); Flam.push_back(lam_e);
    }
  }
  // (2) F^T M F = I, F^T K F = Lambda; (3) the spectrum of line_tables
  const int nmode = (int)Fcol.size(); double lam_max = 0; for (double v : Flam) lam_max = std::max(lam_max, v);
  int nfree = 0; std::vector<double> ref; for (int j = 0; j < nn; ++j) if (T.lam[j] < 1e300) { ++nfree; ref.push_back(T.lam[j]); lam_max = std::max(lam_max, T.lam[j]); }
  if (nmode != nfree || !(lam_max > 0)) { R.why = "mode count differs from the line's"; return R; }
  { std::vector<double> Mf, Kf;
    for (int b = 0; b < nmode; ++b) {
      band(M, Fcol[b], Mf); band(K, Fcol[b], Kf);
      for (int a = 0; a < nmode; ++a) {
        R.orth = std::max(R.orth, std::fabs(dot(Fcol[a], Mf) - (a == b ? 1.0 : 0.0)));
        R.resid = std::max(R.resid, std::fabs(dot(Fcol[a], Kf) - (a == b ? Flam[a] : 0.0)) / lam_max);
      }
    }
    if (!(R.orth <= kTol) || !(R.resid <= kTol)) { R.why = "class-split eigenvectors do not diagonalise the pencil"; return R; } }
  { std::vector<double> mine = Flam; std::sort(mine.begin(), mine.end()); std::sort(ref.begin(), ref.end());
    for (int j = 0; j < nmode; ++j) R.eig_dev = std::max(R.eig_dev, std::fabs(mine[j] - ref[j]) / lam_max);
    if (!(R.eig_dev <= kTol)) { R.why = "eigenvalues differ from the line's"; return R; } }
  for (int p = 0; p < 2; ++p) if (R.grp[p].slots > std::max(R.grp[p].nv, R.grp[p].nm)) { R.why = "more frequencies than class positions"; return R; }
  R.ok = true; return R;
}
// a class transform in fragment order for the class-split pass kernels: `tiles` 16-wide tiles of output rows, `ksteps` k-steps of 4.  Forward [slot][position], backward
// [position][slot] from the SAME entries: the backward matrix is the exact transpose of the forward one
inline std::vector<double> class_fragments(const ClassSplitGroup &G, int cls, int tiles, int ksteps, bool backward) {
  const std::vector<double> &F = cls ? G.Fm : G.Fv; const int np = cls ? G.nm : G.nv, ns = G.slots;
  return backward ? pack_fragments<double>(tiles, ksteps, np, ns, [&](int r, int c) { return F[(size_t)c * np + r]; })
                  : pack_fragments<double>(tiles, ksteps, ns, np, [&](int r, int c) { return F[(size_t)r * np + c]; });
}

// ---- which form the single-rank 3D block FDM of the displacement system can take (PORO_FDM_FORM_PER_DIRECTION) ----
constexpr int kFdmoMaxTiles = 8;       // 16-wide tiles per transformed line the pass kernel of kernels_fdmo.hip is instantiated for: lines of <= 128 entries
// Direction d is SPLIT in parity halves (butterfly in the CG vector kernels, half-size transforms) iff every component has the same end condition at both of its ends and every
// component's eigenvectors came out even or odd there (LineTables::parity: they do on a uniform line with equal ends, not on a graded one); otherwise it is WHOLE (whole-length
// transforms).  len[d] = the transformed length: (n + 1) / 2 or n.  Passes 1 / 3 work on x-y planes and are sized by max(len_x, len_y), pass 2 by len_z.  usable: every
// length fits the kernel; where not, the box keeps the nodal kernels.  all_split: the octant form proper (it keeps its own code path)
struct FdmFormDecision { bool usable = false, all_split = false; int split[3] = {0, 0, 0}, len[3] = {0, 0, 0}; int nt_xy = 0, nt_z = 0, parts = 1; };
inline FdmFormDecision fdm_form_decide(const int fix[3][3][2], const bool parity[3][3] /* [component][direction] */, const int nn[3]) {
  FdmFormDecision D; D.usable = true; D.all_split = true;
  for (int d = 0; d < 3; ++d) {
    bool split = true;
    for (int c = 0; c < 3; ++c) split = split && fix[c][d][0] == fix[c][d][1] && parity[c][d];
    D.split[d] = split ? 1 : 0; D.len[d] = split ? (nn[d] + 1) / 2 : nn[d];
    D.all_split = D.all_split && split; if (split) D.parts *= 2;
    if (nn[d] < 2 || D.len[d] > 16 * kFdmoMaxTiles) D.usable = false;
  }
  D.nt_xy = (std::max(D.len[0], D.len[1]) + 15) / 16; D.nt_z = (D.len[2] + 15) / 16;
  return D;
}

// two matrices side by side, el(r, c, e) with e = 0 / 1, as [block][chunk][k-step u < 4][pair][64][2]: entry e of lane l of (block b, chunk, u, pair p) holds element
// (16 tile(b, p, e) + (l & 15), 4 (4 chunk + u) + (l >> 4)) of matrix e; el returns 0 beyond its matrix
template <class Tile, class El> std::vector<double> pack_paired_chunks(int blocks, int chunks, int pairs, Tile tile, El el) {
  std::vector<double> f((size_t)blocks * chunks * 4 * pairs * 128, 0.0);
  for (int b = 0; b < blocks; ++b) for (int ch = 0; ch < chunks; ++ch) for (int u = 0; u < 4; ++u) for (int p = 0; p < pairs; ++p) for (int l = 0; l < 64; ++l) for (int e = 0; e < 2; ++e) {
    const int r = 16 * tile(b, p, e) + (l & 15), c = 4 * (4 * ch + u) + (l >> 4);
    f[((((size_t)(b * chunks + ch) * 4 + u) * pairs + p) * 64 + l) * 2 + e] = el(r, c, e);
  }
  return f;
}

}  // namespace poro
