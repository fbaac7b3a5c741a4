// Stand-alone check of csrc/cell_field.hpp (host-only): what the per-cell coefficient fields share.  No arguments; the exit code names the first check that failed.
// Built by tests/test_cell_field_cpu.py with -fsanitize=address,undefined and run directly.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "cell_field.hpp"

namespace {
// f() must throw a std::runtime_error whose text is exactly `text`
template <class F> bool refuses(F &&f, const std::string &text) {
  try { f(); } catch (const std::runtime_error &e) { return text == e.what(); }
  return false;
}
// first vertex of the lattice cell (i, j, k) of an nc[0] x nc[1] (x nc[2]) lattice, lexicographic vertex numbering
int32_t first_vertex(const int nc[3], int i, int j, int k) { return (int32_t)((k * (nc[1] + 1) + j) * (nc[0] + 1) + i); }
}  // namespace

int main() {
  // ---- the classification: a layered and a non-layered field on 2 x 1 x 2 cells ----
  const int nc3[3] = {2, 1, 2}; std::vector<double> mean;
  if (!poro::cell_field_layers(3, nc3, {1.0, 1.0, 3.0, 3.0}, mean) || mean[0] != 1.0 || mean[1] != 3.0) return 3;
  if (poro::cell_field_layers(3, nc3, {1.0, 2.0, 3.0, 3.0}, mean) || mean[0] != 1.5 || mean[1] != 3.0) return 4;

  // ---- cell order -> lattice order, the cells in a permuted order, two dofs per cell of which the first counts ----
  {
    const int perm[4] = {2, 0, 3, 1};      // cell e sits on lattice cell perm[e]
    std::vector<int32_t> dofs;
    for (int e = 0; e < 4; ++e) { dofs.push_back(first_vertex(nc3, perm[e] % 2, 0, perm[e] / 2)); dofs.push_back(-7); }
    const std::vector<int64_t> at = poro::cell_lattice_order(3, nc3, dofs.data(), 2, 4, "check");
    for (int e = 0; e < 4; ++e) if (at[e] != perm[e]) return 10;
  }
  const int nc2[3] = {3, 2, 1};
  const int perm2[6] = {4, 2, 0, 5, 1, 3};
  std::vector<int32_t> dofs2;
  for (int e = 0; e < 6; ++e) dofs2.push_back(first_vertex(nc2, perm2[e] % 3, perm2[e] / 3, 0));
  const std::vector<int64_t> order2 = poro::cell_lattice_order(2, nc2, dofs2.data(), 1, 6, "check");
  for (int e = 0; e < 6; ++e) if (order2[e] != perm2[e]) return 11;
  // the two refusals: a cell that starts on the last vertex of a lattice line (x, y, and z in 3D), two cells on one lattice cell
  for (int32_t bad : {first_vertex(nc2, 3, 0, 0), first_vertex(nc2, 0, 2, 0)}) {
    std::vector<int32_t> d = dofs2; d[4] = bad;
    if (!refuses([&] { poro::cell_lattice_order(2, nc2, d.data(), 1, 6, "poro_ctx_set_cell_permeability"); }, "poro_ctx_set_cell_permeability: cell 4 does not start at a lattice cell's first vertex")) return 12;
  }
  {
    const int32_t d[2] = {0, first_vertex(nc3, 0, 0, 2)};
    if (!refuses([&] { poro::cell_lattice_order(3, nc3, d, 1, 2, "poro_ctx_set_cell_moduli"); }, "poro_ctx_set_cell_moduli: cell 1 does not start at a lattice cell's first vertex")) return 13;
    std::vector<int32_t> twice = dofs2; twice[5] = twice[1];
    if (!refuses([&] { poro::cell_lattice_order(2, nc2, twice.data(), 1, 6, "poro_ctx_set_cell_moduli"); }, "poro_ctx_set_cell_moduli: two cells on one lattice cell")) return 14;
  }

  // ---- the field state: two components on 3 x 2 cells in the permuted order, the first layered (1 | 2), the second not ----
  {
    const double by_lattice[2][6] = {{1, 1, 1, 2, 2, 2}, {5, 5, 5, 5, 6, 7}};
    double a[6], b[6];
    for (int e = 0; e < 6; ++e) { a[e] = by_lattice[0][perm2[e]]; b[e] = by_lattice[1][perm2[e]]; }
    poro::CellField<2> F;
    const auto lattice = F.set({a, b}, 6, &order2, 2, nc2);
    if (F.kind != 2) return 20;
    for (int e = 0; e < 6; ++e) if (F.host[0][e] != a[e] || F.host[1][e] != b[e] || lattice[0][e] != by_lattice[0][e] || lattice[1][e] != by_lattice[1][e]) return 21;
    if (F.layer[0] != std::vector<double>{1.0, 2.0} || F.layer[1] != std::vector<double>{5.0, 6.0}) return 22;      // the value, the mean in index order
    const auto both = F.set({a, a}, 6, &order2, 2, nc2);
    if (F.kind != 1 || F.layer[1] != std::vector<double>{1.0, 2.0} || both[1] != lattice[0]) return 23;
    // without a lattice: general, no layers, no lattice copies
    const auto none = F.set({a, b}, 6);
    if (F.kind != 2 || !F.layer[0].empty() || !F.layer[1].empty() || !none[0].empty() || F.host[1][5] != b[5]) return 24;
    F.clear();
    if (F.kind != 0 || !F.host[0].empty() || !F.host[1].empty()) return 25;
    poro::CellField<1> one;
    one.set({a}, 6, &order2, 2, nc2);
    if (one.kind != 1 || one.layer[0] != std::vector<double>{1.0, 2.0}) return 26;
  }

  // ---- layers by cell centres: 3 x 2 unit cells (y slowest) and 2 x 1 x 2 cells of height 0.5 (z slowest) ----
  {
    std::vector<double> X; std::vector<int32_t> cells;
    for (int j = 0; j <= 2; ++j) for (int i = 0; i <= 3; ++i) { X.push_back(i); X.push_back(j); }
    for (int j = 0; j < 2; ++j) for (int i = 0; i < 3; ++i) for (int v = 0; v < 4; ++v) cells.push_back((j + v / 2) * 4 + i + v % 2);
    const double tops[2] = {0.5, 2.0}, on_the_centre[2] = {0.5, 1.5}, low[1] = {1.0};
    if (poro::cell_layers_by_centre(X, cells, 2, 2, tops, "check") != std::vector<int>{0, 0, 0, 1, 1, 1}) return 30;
    if (poro::cell_layers_by_centre(X, cells, 2, 2, on_the_centre, "check") != std::vector<int>{0, 0, 0, 1, 1, 1}) return 31;      // top >= centre: a centre on a top belongs below
    if (!refuses([&] { poro::cell_layers_by_centre(X, cells, 2, 1, low, "set_moduli_layers"); },
                 "set_moduli_layers: the centre of cell 3 (" + std::to_string(1.5) + ") lies above every layer top")) return 32;
    std::vector<double> X3; std::vector<int32_t> cells3;
    for (int k = 0; k <= 2; ++k) for (int j = 0; j <= 1; ++j) for (int i = 0; i <= 2; ++i) { X3.push_back(i); X3.push_back(j); X3.push_back(0.5 * k); }
    for (int k = 0; k < 2; ++k) for (int i = 0; i < 2; ++i) for (int v = 0; v < 8; ++v) cells3.push_back(((k + v / 4) * 2 + (v / 2) % 2) * 3 + i + v % 2);
    const double tops3[3] = {0.1, 0.3, 0.9};
    if (poro::cell_layers_by_centre(X3, cells3, 3, 3, tops3, "check") != std::vector<int>{1, 1, 2, 2}) return 33;
  }

  // ---- inheritance through coarse cells: bit-equal contributors give the value itself, differing ones their mean ----
  {
    const double third = 1.0 / 3.0;
    const std::vector<int32_t> old_coarse = {0, 1, 1, 1, 1, 2, 2, 2, 2}, new_coarse = {0, 0, 0, 0, 1, 2, 2};
    const std::vector<double> old_value = {0.1, third, third, third, third, 1.0, 2.0, 3.0, 5.0};
    const std::vector<double> got = poro::cell_field_inherit(old_coarse, old_value, new_coarse, 3);
    if (got != std::vector<double>{0.1, 0.1, 0.1, 0.1, third, 2.75, 2.75}) return 40;
    const std::vector<double> tenths(8, 0.1); const std::vector<int32_t> eight(8, 0);
    if (poro::cell_field_inherit(eight, tenths, {0}, 1) != std::vector<double>{0.1}) return 41;      // (the sum of eight 0.1 divided by 8 is not 0.1)
  }
  std::puts("cell_field_check ok");
  return 0;
}
