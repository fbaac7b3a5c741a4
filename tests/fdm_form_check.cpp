// Stand-alone check of the form decision of the block FDM (csrc/fdm_tables.hpp: fdm_form_decide, whole_line_fragments; host only, no HIP): prints one JSON line per case;
// tests/test_fdm_form_cpu.py compiles, runs and asserts.
// Arguments, one per box: "name:nx,ny,nz:k:gx,gy,gz:label.comp,label.comp,..." - cells, degree, grading per direction (0 = uniform) and the Dirichlet list
// (face label 2 d + side fixes component comp).  The tile-count and packing cases are built in.
#include "../poroelasticity_dealii_amd/csrc/fdm_tables.hpp"
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

using namespace poro;

// cell sizes of n cells on [0, 10]: uniform, or graded as the graded-box builder does (x = L expm1(g t) / expm1(g))
static std::vector<double> cells_of(int cells, double grading) {
  std::vector<double> x(cells + 1), h(cells);
  for (int i = 0; i <= cells; ++i) { const double t = (double)i / cells; x[i] = grading != 0.0 ? 10.0 * std::expm1(grading * t) / std::expm1(grading) : 10.0 * t; }
  for (int i = 0; i < cells; ++i) h[i] = x[i + 1] - x[i];
  return h;
}
static std::vector<std::string> split_at(const std::string &s, char sep) {
  std::vector<std::string> out; std::stringstream ss(s); std::string item;
  while (std::getline(ss, item, sep)) out.push_back(item);
  return out;
}
static void print_decision(const char *kind, const std::string &name, const FdmFormDecision &D) {
  std::printf("{\"case\": \"%s\", \"name\": \"%s\", \"usable\": %d, \"all_split\": %d, \"split\": [%d, %d, %d], \"len\": [%d, %d, %d], \"nt_xy\": %d, \"nt_z\": %d, \"parts\": %d}\n", kind, name.c_str(),
              (int)D.usable, (int)D.all_split, D.split[0], D.split[1], D.split[2], D.len[0], D.len[1], D.len[2], D.nt_xy, D.nt_z, D.parts);
}

// the decision for a box as build_fdm_u makes it: fix flags from the list, LineTables::parity of every (component, direction) from the tables themselves
static void box_case(const std::string &arg) {
  const std::vector<std::string> f = split_at(arg, ':');
  if (f.size() != 5) { std::fprintf(stderr, "bad case %s\n", arg.c_str()); std::exit(2); }
  const std::vector<std::string> n = split_at(f[1], ','), g = split_at(f[3], ','), bc = split_at(f[4], ',');
  const int k = std::atoi(f[2].c_str());
  int fix[3][3][2] = {}; bool parity[3][3]; int nn[3];
  for (const std::string &e : bc) { const std::vector<std::string> lc = split_at(e, '.'); const int label = std::atoi(lc[0].c_str()), comp = std::atoi(lc[1].c_str()); fix[comp][label / 2][label % 2] = 1; }
  for (int d = 0; d < 3; ++d) {
    const int cells = std::atoi(n[d].c_str()); nn[d] = k * cells + 1;
    for (int c = 0; c < 3; ++c) parity[c][d] = line_tables(k, cells_of(cells, std::atof(g[d].c_str())), fix[c][d][0] != 0, fix[c][d][1] != 0).parity;
  }
  print_decision("box", f[0], fdm_form_decide(fix, parity, nn));
}

// tile counts: a line of `len` transformed entries in direction d, whole (one-sided end, no parity) or split (equal ends, parity; 2 len - 1 nodes), the other two directions 5 nodes, split
static void tiles_case(int len, int d, bool split) {
  int fix[3][3][2] = {}; bool parity[3][3]; int nn[3] = {5, 5, 5};
  for (int c = 0; c < 3; ++c) for (int e = 0; e < 3; ++e) { fix[c][e][0] = fix[c][e][1] = (c == e); parity[c][e] = true; }
  nn[d] = split ? 2 * len - 1 : len;
  if (!split) { fix[d][d][1] = 0; for (int c = 0; c < 3; ++c) parity[c][d] = (c != d); }
  print_decision("tiles", std::string(split ? "split" : "whole") + "_" + "xyz"[d] + "_" + std::to_string(len), fdm_form_decide(fix, parity, nn));
}

// whole-length fragments of a line: unpacked through the lane map of pack_fragments they are S^T (forward) and S (backward) exactly, zero beyond the line
static void pack_case(const char *name, int k, int cells, bool fix_lo, bool fix_hi, double grading, int tiles) {
  const LineTables T = line_tables(k, cells_of(cells, grading), fix_lo, fix_hi);
  const int n = T.n; long mismatch = 0, pad_nonzero = 0, sizes_ok = 1;
  for (int backward = 0; backward < 2; ++backward) {
    const std::vector<double> F = whole_line_fragments(T, tiles, backward != 0);
    if (F.size() != (size_t)tiles * 4 * tiles * 64) sizes_ok = 0;
    for (int t = 0; t < tiles; ++t) for (int kk = 0; kk < 4 * tiles; ++kk) for (int l = 0; l < 64; ++l) {
      const int r = 16 * t + (l & 15), c = 4 * kk + (l >> 4); const double v = F[((size_t)t * 4 * tiles + kk) * 64 + l];
      if (r < n && c < n) { const double want = backward ? T.S[(size_t)r * n + c] : T.S[(size_t)c * n + r]; if (v != want) ++mismatch; }
      else if (v != 0.0) ++pad_nonzero;
    }
  }
  std::printf("{\"case\": \"pack\", \"name\": \"%s\", \"n\": %d, \"parity\": %d, \"sizes_ok\": %ld, \"mismatch\": %ld, \"pad_nonzero\": %ld}\n", name, n, (int)T.parity, sizes_ok, mismatch, pad_nonzero);
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) box_case(argv[i]);
  for (int len : {16, 17, 80, 81, 128, 129}) for (int d = 0; d < 3; ++d) for (int split = 0; split < 2; ++split) tiles_case(len, d, split != 0);
  pack_case("q2_17_lo", 2, 8, true, false, 0.0, 2);
  pack_case("q2_33_hi", 2, 16, false, true, 0.0, 3);
  pack_case("q1_16_graded", 1, 15, true, true, -0.7, 1);
  pack_case("q2_73_lo", 2, 36, true, false, 0.0, 5);
  return 0;
}
