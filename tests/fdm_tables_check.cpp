// Stand-alone check of csrc/fdm_tables.hpp (host only, no HIP): prints one JSON line per case; tests/test_fdm_tables_cpu.py compiles, runs and asserts.
// Also the sanitizer target of the header: g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined.
#include "../poroelasticity_dealii_amd/csrc/fdm_tables.hpp"
#include <cstdio>
#include <string>

using namespace poro;

// vertices of n cells on [0, 10]: uniform, or graded as the graded-box builder does (x = L expm1(g t) / expm1(g))
static std::vector<double> grid_of(int cells, double grading) {
  std::vector<double> x(cells + 1);
  for (int i = 0; i <= cells; ++i) { const double t = (double)i / cells; x[i] = grading != 0.0 ? 10.0 * std::expm1(grading * t) / std::expm1(grading) : 10.0 * t; }
  return x;
}
static void print_vec(const char *name, const std::vector<double> &v, size_t n) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]");
}

static void line_case(int k, int cells, bool fix_lo, bool fix_hi, double grading) {
  const std::vector<double> x = grid_of(cells, grading);
  std::vector<double> hc(cells); for (int i = 0; i < cells; ++i) hc[i] = x[i + 1] - x[i];
  const LineTables T = line_tables(k, hc, fix_lo, fix_hi);
  const int nn = T.n, f0 = fix_lo ? 1 : 0, nf = nn - f0 - (fix_hi ? 1 : 0);
  const std::vector<double> &S = T.S;
  std::vector<double> M, K; fe1d(k, hc, M, K);
  // S^T M S and S^T K S on the free modes, through the band of M and K
  double orth = 0, resid = 0, lam_max = 0;
  for (int j = 0; j < nf; ++j) lam_max = std::max(lam_max, T.lam[j]);
  std::vector<double> St((size_t)nf * nn), MS((size_t)nf * nn, 0.0), KS((size_t)nf * nn, 0.0);      // mode-major: contiguous dot products below
  for (int j = 0; j < nf; ++j) for (int i = 0; i < nn; ++i) St[(size_t)j * nn + i] = S[(size_t)i * nn + j];
  for (int j = 0; j < nf; ++j) for (int i = 0; i < nn; ++i) for (int p = std::max(0, i - 2 * k); p <= std::min(nn - 1, i + 2 * k); ++p) {
    MS[(size_t)j * nn + i] += M[(size_t)i * nn + p] * St[(size_t)j * nn + p]; KS[(size_t)j * nn + i] += K[(size_t)i * nn + p] * St[(size_t)j * nn + p];
  }
  for (int a = 0; a < nf; ++a) for (int b = 0; b < nf; ++b) {
    double m = 0, s = 0;
    for (int i = 0; i < nn; ++i) { m += St[(size_t)a * nn + i] * MS[(size_t)b * nn + i]; s += St[(size_t)a * nn + i] * KS[(size_t)b * nn + i]; }
    orth = std::max(orth, std::fabs(m - (a == b ? 1.0 : 0.0))); resid = std::max(resid, std::fabs(s - (a == b ? T.lam[a] : 0.0)));
  }
  // structure: zero rows at removed nodes, zero columns and lam = inf behind the free modes
  bool rows_zero = true, cols_zero = true, lam_inf = true;
  for (int j = 0; j < nn; ++j) { if (fix_lo && S[j] != 0.0) rows_zero = false; if (fix_hi && S[(size_t)(nn - 1) * nn + j] != 0.0) rows_zero = false; }
  for (int j = nf; j < nn; ++j) { for (int i = 0; i < nn; ++i) if (S[(size_t)i * nn + j] != 0.0) cols_zero = false; if (!std::isinf(T.lam[j])) lam_inf = false; }
  // parity, mode by mode with the test of the classification (no early exit), and the mirror defect max_k |s_k -+ s_(n-1-k)| of the modes it accepts
  int n_even = 0, n_odd = 0, n_neither = 0; double mirror = 0;
  for (int m = 0; m < nf; ++m) {
    double ds = 0, da = 0, nrm = 0, es = 0, ea = 0;
    for (int i = 0; i < nn; ++i) { const double a = S[(size_t)i * nn + m], b = S[(size_t)(nn - 1 - i) * nn + m]; ds += (a - b) * (a - b); da += (a + b) * (a + b); nrm += a * a; es = std::max(es, std::fabs(a - b)); ea = std::max(ea, std::fabs(a + b)); }
    if (ds <= 1e-20 * nrm) { ++n_even; mirror = std::max(mirror, es); } else if (da <= 1e-20 * nrm) { ++n_odd; mirror = std::max(mirror, ea); } else ++n_neither;
  }
  std::printf("{\"case\": \"line\", \"k\": %d, \"cells\": %d, \"fix_lo\": %d, \"fix_hi\": %d, \"grading\": %.17g, \"n\": %d, \"n_free\": %d, \"orth\": %.3e, \"resid\": %.3e, "
              "\"rows_zero\": %d, \"cols_zero\": %d, \"lam_inf\": %d, \"parity\": %d, \"even\": %zu, \"odd\": %zu, \"modes_even\": %d, \"modes_odd\": %d, \"modes_neither\": %d, \"mirror\": %.17g, ",
              k, cells, (int)fix_lo, (int)fix_hi, grading, nn, nf, orth, lam_max > 0 ? resid / lam_max : resid, (int)rows_zero, (int)cols_zero, (int)lam_inf, (int)T.parity, T.even.size(), T.odd.size(),
              n_even, n_odd, n_neither, mirror);
  print_vec("grid", x, x.size()); std::printf(", "); print_vec("lam", T.lam, (size_t)std::max(nf, 0));
  if (k == 1 && !fix_lo && !fix_hi && grading == 0.0) { std::printf(", "); const LineTables Q = q1_eig(cells, hc[0]); print_vec("lam_q1", Q.lam, Q.lam.size()); std::printf(", \"parity_q1\": %d", (int)Q.parity); }
  std::printf("}\n");
}

// ---- packers: unpack every entry of a buffer by the documented lane map and compare with the source ----
struct Tally { long mismatch = 0, pad_nonzero = 0, uncovered = 0; };
static void report(const std::string &name, size_t size, size_t expected_size, const Tally &t) {
  std::printf("{\"case\": \"pack\", \"name\": \"%s\", \"size\": %zu, \"expected_size\": %zu, \"mismatch\": %ld, \"pad_nonzero\": %ld, \"uncovered\": %ld}\n", name.c_str(), size, expected_size, t.mismatch, t.pad_nonzero,
              t.uncovered);
}
// source matrices with entries that are all different, non-zero and exact in fp32 as well
static double src(int r, int c, int e) { return (e ? -1.0 : 1.0) * (1.0 + r * 1024.0 + c); }

// [tile][k-step][64]: entry ((t ksteps + kk) 64 + l) is element (16 t + (l & 15), 4 kk + (l >> 4)), zero beyond rows x cols
template <class T> static void check_fragments(const std::string &name, int tiles, int ksteps, int rows, int cols) {
  const std::vector<T> f = pack_fragments<T>(tiles, ksteps, rows, cols, [](int r, int c) { return src(r, c, 0); });
  Tally t; std::vector<int> hit((size_t)rows * cols, 0);
  for (size_t at = 0; at < f.size(); ++at) {
    const int l = (int)(at % 64), kk = (int)(at / 64 % ksteps), tile = (int)(at / 64 / ksteps), r = 16 * tile + (l & 15), c = 4 * kk + (l >> 4);
    if (r < rows && c < cols) { if (f[at] != (T)src(r, c, 0)) ++t.mismatch; ++hit[(size_t)r * cols + c]; } else if (f[at] != (T)0) ++t.pad_nonzero;
  }
  for (int h : hit) if (h != 1) ++t.uncovered;
  report(name, f.size(), (size_t)tiles * ksteps * 64, t);
}
// [block][chunk][u < 4][pair][64][2]: entry e of lane l of (b, ch, u, p) is element (16 tile(b, p, e) + (l & 15), 4 (4 ch + u) + (l >> 4)) of matrix e (rows[e] x cols[e])
template <class Tile> static void check_paired(const std::string &name, int blocks, int chunks, int pairs, Tile tile, const int rows[2], const int cols[2], bool one_matrix) {
  auto el = [&](int r, int c, int e) { const int m = one_matrix ? 0 : e; return r < rows[m] && c < cols[m] ? src(r, c, m) : 0.0; };
  const std::vector<double> f = pack_paired_chunks(blocks, chunks, pairs, tile, el);
  Tally t; std::vector<int> hit[2]; for (int e = 0; e < 2; ++e) hit[e].assign((size_t)rows[e] * cols[e], 0);
  for (size_t at = 0; at < f.size(); ++at) {
    size_t q = at; const int e = (int)(q % 2); q /= 2; const int l = (int)(q % 64); q /= 64; const int p = (int)(q % pairs); q /= pairs; const int u = (int)(q % 4); q /= 4;
    const int ch = (int)(q % chunks), b = (int)(q / chunks), m = one_matrix ? 0 : e;
    const int r = 16 * tile(b, p, e) + (l & 15), c = 4 * (4 * ch + u) + (l >> 4);
    if (r < rows[m] && c < cols[m]) { if (f[at] != src(r, c, m)) ++t.mismatch; ++hit[m][(size_t)r * cols[m] + c]; } else if (f[at] != 0.0) ++t.pad_nonzero;
  }
  for (int m = 0; m < (one_matrix ? 1 : 2); ++m) for (int h : hit[m]) if (h != 1) ++t.uncovered;
  report(name, f.size(), (size_t)blocks * chunks * 4 * pairs * 128, t);
}

int main() {
  const struct { int k, cells, lo, hi; double g; } lines[] = {
      {1, 1, 0, 0, 0}, {1, 2, 1, 0, 0}, {2, 1, 1, 1, 0}, {2, 2, 0, 0, 0}, {2, 48, 0, 0, 0}, {2, 48, 1, 1, 0}, {2, 49, 1, 1, 0}, {2, 49, 1, 0, 0}, {1, 97, 0, 0, 0},
      {2, 48, 1, 1, 0.5}, {2, 64, 1, 0, -0.7}, {2, 335, 0, 0, 0}, {2, 335, 1, 1, 0}};
  for (const auto &c : lines) line_case(c.k, c.cells, c.lo != 0, c.hi != 0, c.g);

  // nodal forms of a line of nn points.  Register form: nch chunks of 16 columns, tile pairs 2p + e of the one matrix; LDS form: [MT][KK][64] in fp64 and fp32
  for (int nn : {11, 145}) {          // nch = 1, 10
    const int nch = (nn + 15) / 16, rc[2] = {nn, nn};
    check_paired("nodal_reg_" + std::to_string(nn), 1, nch, (nch + 1) / 2, [](int, int p, int e) { return 2 * p + e; }, rc, rc, true);
    check_fragments<double>("nodal_lds_f64_" + std::to_string(nn), (nn + 15) / 16, (nn + 3) / 4, nn, nn);
    check_fragments<float>("nodal_lds_f32_" + std::to_string(nn), (nn + 15) / 16, (nn + 3) / 4, nn, nn);
  }
  // split form: the even (ceil(nn / 2) modes) and the odd (floor(nn / 2)) matrix side by side, forward modes x half line, backward half line x modes
  for (int nn : {11, 145}) {          // nch = 1, 5
    const int h = (nn + 1) / 2, nch = (h + 15) / 16, modes[2] = {h, nn / 2}, half[2] = {h, h};
    check_paired("split_fwd_" + std::to_string(nn), 1, nch, nch, [](int, int p, int) { return p; }, modes, half, false);
    check_paired("split_bwd_" + std::to_string(nn), 1, nch, nch, [](int, int p, int) { return p; }, half, modes, false);
  }
  // blocked split form: row blocks of 5 tiles per parity
  for (int nn : {163, 671}) {
    const int h = (nn + 1) / 2, modes[2] = {h, nn / 2}, half[2] = {h, h};
    for (int w = 0; w < 2; ++w) {
      const int rows = h, cols = h, kk = (cols + 3) / 4, nchk = (kk + 3) / 4, mb = (rows + 79) / 80;
      check_paired(std::string(w ? "blocked_bwd_" : "blocked_fwd_") + std::to_string(nn), mb, nchk, 5, [](int b, int p, int) { return 5 * b + p; }, w ? half : modes, w ? modes : half, false);
    }
  }
  // octant form: [nt][4 nt][64], a parity group's modes x half line and back
  for (int nt : {1, 5, 8}) {
    const int h = nt == 1 ? 6 : 16 * nt - (nt == 5 ? 7 : 0);      // half lines of 6, 73 and 128 entries
    check_fragments<double>("octant_fwd_nt" + std::to_string(nt), nt, 4 * nt, h - 1, h);
    check_fragments<double>("octant_bwd_nt" + std::to_string(nt), nt, 4 * nt, h, h - 1);
  }
  return 0;
}
