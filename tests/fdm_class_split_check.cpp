// Stand-alone check of the class-split tables of csrc/fdm_tables.hpp (host only, no HIP): prints one JSON line per line case; tests/test_fdm_class_split_cpu.py compiles,
// runs and asserts.  Also a sanitizer target: g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined.
#include "../poroelasticity_dealii_amd/csrc/fdm_tables.hpp"
#include <cstdio>

using namespace poro;

static std::vector<double> grid_of(int cells, double grading) {
  std::vector<double> x(cells + 1);
  for (int i = 0; i <= cells; ++i) { const double t = (double)i / cells; x[i] = grading != 0.0 ? 10.0 * std::expm1(grading * t) / std::expm1(grading) : 10.0 * t; }
  return x;
}
static void print_vec(const char *name, const std::vector<double> &v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]");
}
// fragments of a class transform, unpacked by the documented lane map, against the table; the backward set against the transpose of the forward one, entry by entry
static void fragment_check(const ClassSplitGroup &G, int cls, long &mismatch, long &pad_nonzero, long &not_transposed) {
  const int np = cls ? G.nm : G.nv, ns = G.slots, nt = (std::max(G.nv, 1) + 7) / 8, tiles = (nt + 1) / 2, ksteps = 2 * nt;      // the kernel's sizes: nt tiles per half line
  const std::vector<double> &F = cls ? G.Fm : G.Fv;
  const std::vector<double> fw = class_fragments(G, cls, tiles, ksteps, false), bw = class_fragments(G, cls, tiles, ksteps, true);
  if (fw.size() != (size_t)tiles * ksteps * 64 || bw.size() != fw.size()) { ++mismatch; return; }
  std::vector<double> A((size_t)16 * tiles * 4 * ksteps, 0.0), B = A;       // dense [row][column] images of both
  for (size_t at = 0; at < fw.size(); ++at) {
    const int l = (int)(at % 64), kk = (int)(at / 64 % ksteps), t = (int)(at / 64 / ksteps), r = 16 * t + (l & 15), c = 4 * kk + (l >> 4);
    A[(size_t)r * 4 * ksteps + c] = fw[at]; B[(size_t)r * 4 * ksteps + c] = bw[at];
    if (r < ns && c < np) { if (fw[at] != F[(size_t)r * np + c]) ++mismatch; } else if (fw[at] != 0.0) ++pad_nonzero;
    if (r < np && c < ns) { if (bw[at] != F[(size_t)c * np + r]) ++mismatch; } else if (bw[at] != 0.0) ++pad_nonzero;
  }
  const int dim = std::min(16 * tiles, 4 * ksteps);
  for (int r = 0; r < dim; ++r) for (int c = 0; c < dim; ++c) if (A[(size_t)r * 4 * ksteps + c] != B[(size_t)c * 4 * ksteps + r]) ++not_transposed;
}

static void line_case(int k, int cells, bool fix_lo, bool fix_hi, double grading) {
  const std::vector<double> x = grid_of(cells, grading);
  std::vector<double> hc(cells); for (int i = 0; i < cells; ++i) hc[i] = x[i + 1] - x[i];
  const LineTables T = line_tables(k, hc, fix_lo, fix_hi);
  const ClassSplitTables R = class_split_tables(k, hc, fix_lo, fix_hi, T);
  std::printf("{\"k\": %d, \"cells\": %d, \"fix_lo\": %d, \"fix_hi\": %d, \"grading\": %.17g, \"n\": %d, \"ok\": %d, \"why\": \"%s\", \"off_block\": %.3e, \"orth\": %.3e, \"resid\": %.3e, \"eig_dev\": %.3e, ",
              k, cells, (int)fix_lo, (int)fix_hi, grading, T.n, (int)R.ok, R.why, R.off_block, R.orth, R.resid, R.eig_dev);
  print_vec("grid", x);
  if (R.ok) {
    // the full-line eigenvectors the tables stand for, mode by mode in the kernels' order [parity][class][slot]: node values through the mirror symmetry of the group
    const int nn = T.n, h = (nn + 1) / 2;
    std::vector<double> F, lam; long mismatch = 0, pad_nonzero = 0, not_transposed = 0;
    std::printf(", \"groups\": [");
    for (int p = 0; p < 2; ++p) {
      const ClassSplitGroup &G = R.grp[p]; int present[2] = {0, 0};
      for (int e = 0; e < 2; ++e) for (int s = 0; s < G.slots; ++s) {
        const double l = e ? G.lam_m[s] : G.lam_v[s];
        if (!(l < 1e300)) continue;
        ++present[e]; lam.push_back(l);
        std::vector<double> f(nn, 0.0);
        for (int i = 0; i < h; ++i) {
          const int q = i / 2; const double v = (i & 1) ? G.mix[4 * s + 2 * e + 1] * G.Fm[(size_t)s * G.nm + q] : G.mix[4 * s + 2 * e] * G.Fv[(size_t)s * G.nv + q];
          f[i] = v; if (nn - 1 - i != i) f[nn - 1 - i] = p ? -v : v;
        }
        F.insert(F.end(), f.begin(), f.end());
      }
      fragment_check(G, 0, mismatch, pad_nonzero, not_transposed); fragment_check(G, 1, mismatch, pad_nonzero, not_transposed);
      std::printf("%s{\"nv\": %d, \"nm\": %d, \"slots\": %d, \"modes_v\": %d, \"modes_m\": %d}", p ? ", " : "", G.nv, G.nm, G.slots, present[0], present[1]);
    }
    std::printf("], \"frag_mismatch\": %ld, \"frag_pad_nonzero\": %ld, \"frag_not_transposed\": %ld, ", mismatch, pad_nonzero, not_transposed);
    print_vec("lam", lam); std::printf(", "); print_vec("F", F);
  }
  std::printf("}\n");
}

int main() {
  for (int cells : {1, 2, 5, 6, 8, 32, 33, 64, 72, 96}) for (int fix = 0; fix < 2; ++fix) line_case(2, cells, fix != 0, fix != 0, 0.0);
  line_case(2, 48, true, true, 0.5); line_case(2, 48, false, false, -0.7);      // graded
  line_case(2, 49, true, false, 0.0); line_case(2, 6, false, true, 0.0);        // different ends
  line_case(1, 48, false, false, 0.0); line_case(1, 7, true, true, 0.0);        // Q1
  return 0;
}
