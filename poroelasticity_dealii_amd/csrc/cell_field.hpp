// Host-only: what every per-cell coefficient field has in common, whichever coefficient it holds (k / mu of the pressure system: poro_ctx_set_cell_permeability; Lame
// lambda and shear G of the displacement system: poro_ctx_set_cell_moduli).  The classification of a field on a tensor-product lattice, the caller's cell order -> lattice
// order, the host state a context keeps per field, and the two loops of the host layer (layers by cell centres, inheritance through the coarse cells of refined boxes).
// No HIP, no project header: compiles into the device library, the host layer and stand-alone checks alike.  Refusals are std::runtime_error
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace poro {

// A field in lattice cell order (x fastest) on nc[0] x nc[1] (x nc[2]) cells: is it constant within every layer of the slowest direction (exact equality)?  layer_mean
// gets the arithmetic mean of every layer (the layer's value where the answer is yes)
inline bool cell_field_layers(int dim, const int nc[3], const std::vector<double> &lattice, std::vector<double> &layer_mean) {
  const int64_t per_layer = dim == 3 ? (int64_t)nc[0] * nc[1] : nc[0];
  const int n_layers = nc[dim - 1];
  layer_mean.assign((size_t)n_layers, 0.0);
  bool layered = true;
  for (int k = 0; k < n_layers; ++k) {
    const double *v = lattice.data() + (size_t)k * per_layer;
    double sum = 0;
    for (int64_t i = 0; i < per_layer; ++i) { sum += v[i]; if (v[i] != v[0]) layered = false; }
    layer_mean[k] = sum / (double)per_layer;
  }
  if (layered) for (int k = 0; k < n_layers; ++k) layer_mean[k] = lattice[(size_t)k * per_layer];
  return layered;
}

// Boxes and tensor-product grids: the caller's cell order -> lattice order through every cell's first vertex (= its first pressure dof, lexicographic numbering on
// (nc[0] + 1) x (nc[1] + 1) (x (nc[2] + 1)) vertices).  first_dof[e * stride] is cell e's; the answer is the lattice index (x fastest) of every cell.  `who` names the
// calling entry point in the refusals
inline std::vector<int64_t> cell_lattice_order(int dim, const int nc[3], const int32_t *first_dof, int64_t stride, int64_t n_cells, const char *who) {
  const int64_t np0 = nc[0] + 1, np1 = nc[1] + 1, n2 = dim == 3 ? nc[2] : 1;
  std::vector<int64_t> at((size_t)n_cells);
  std::vector<uint8_t> seen((size_t)(nc[0] * (int64_t)nc[1] * n2), 0);
  for (int64_t e = 0; e < n_cells; ++e) {
    const int64_t v = first_dof[e * stride];
    const int64_t i = v % np0, j = (v / np0) % np1, k = dim == 3 ? v / (np0 * np1) : 0;
    if (v < 0 || i >= nc[0] || j >= nc[1] || k >= n2) throw std::runtime_error(std::string(who) + ": cell " + std::to_string(e) + " does not start at a lattice cell's first vertex");
    at[e] = (k * nc[1] + j) * nc[0] + i;
    if (seen[at[e]]) throw std::runtime_error(std::string(who) + ": two cells on one lattice cell");
    seen[at[e]] = 1;
  }
  return at;
}

// The host state of a field of N components.  kind: 0 none, 1 every component constant within every cell layer of the slowest lattice direction, 2 general.  host: the
// caller's arrays in the caller's cell order.  layer: per cell layer the value (a layered component) or the arithmetic mean; empty without a lattice
template <int N> struct CellField {
  int kind = 0;
  std::vector<double> host[N], layer[N];
  void clear() { kind = 0; for (int a = 0; a < N; ++a) { host[a].clear(); layer[a].clear(); } }
  // Takes the first `used` of the N arrays of n_cells values; the components past them stay empty and do not enter `kind`.  order (cell_lattice_order on dim, nc; null:
  // no lattice, kind 2): classifies every component and returns the lattice-ordered copies (empty without a lattice)
  std::array<std::vector<double>, N> set(const double *const (&comp)[N], int64_t n_cells, const std::vector<int64_t> *order = nullptr, int dim = 0, const int *nc = nullptr, int used = N) {
    std::array<std::vector<double>, N> lattice;
    kind = order ? 1 : 2;
    for (int a = used; a < N; ++a) { host[a].clear(); layer[a].clear(); }
    for (int a = 0; a < used; ++a) {
      host[a].assign(comp[a], comp[a] + n_cells); layer[a].clear();
      if (!order) continue;
      lattice[a].assign((size_t)nc[0] * nc[1] * (dim == 3 ? nc[2] : 1), 0.0);
      for (int64_t e = 0; e < n_cells; ++e) lattice[a][(size_t)(*order)[e]] = host[a][e];
      if (!cell_field_layers(dim, nc, lattice[a], layer[a])) kind = 2;
    }
    return lattice;
  }
};

// Layers along the slowest direction (z in 3D, y in 2D): every cell's layer is the first whose top is >= the coordinate of the cell's centre there.  vertices:
// [n_vertices][dim], cells: [n_cells][2^dim] vertex indices
inline std::vector<int> cell_layers_by_centre(const std::vector<double> &vertices, const std::vector<int32_t> &cells, int dim, int n_layers, const double *top, const char *who) {
  const int nv = 1 << dim; const int64_t nc = (int64_t)cells.size() / nv;
  std::vector<int> layer((size_t)nc);
  for (int64_t c = 0; c < nc; ++c) {
    double z = 0;
    for (int v = 0; v < nv; ++v) z += vertices[(size_t)cells[c * nv + v] * dim + (dim - 1)];
    z /= nv;
    int l = 0;
    while (l < n_layers && !(top[l] >= z)) ++l;
    if (l == n_layers) throw std::runtime_error(std::string(who) + ": the centre of cell " + std::to_string(c) + " (" + std::to_string(z) + ") lies above every layer top");
    layer[(size_t)c] = l;
  }
  return layer;
}

// A field on the cells of one refined box, carried to another refined box over the same ncoarse coarse cells: every cell takes the value of its coarse cell - a child its
// parent's, a parent the mean of its children.  One contributor, or several bit-equal ones: the value itself, exactly; the mean is formed only where they differ
inline std::vector<double> cell_field_inherit(const std::vector<int32_t> &old_coarse, const std::vector<double> &old_value, const std::vector<int32_t> &new_coarse, size_t ncoarse) {
  std::vector<double> sum(ncoarse, 0.0), first(ncoarse, 0.0); std::vector<int> cnt(ncoarse, 0); std::vector<uint8_t> same(ncoarse, 1);
  for (size_t c = 0; c < old_coarse.size(); ++c) {
    const int32_t cc = old_coarse[c]; const double v = old_value[c];
    if (!cnt[cc]) first[cc] = v; else if (v != first[cc]) same[cc] = 0;
    sum[cc] += v; cnt[cc]++;
  }
  std::vector<double> out(new_coarse.size());
  for (size_t c = 0; c < new_coarse.size(); ++c) { const int32_t cc = new_coarse[c]; out[c] = same[cc] ? first[cc] : sum[cc] / cnt[cc]; }
  return out;
}

}  // namespace poro
