// Hybrid operator form on refined boxes (poro_ctx_set_operator_form, PORO_OPFORM_HYBRID): the plan derived on the host from what the context already holds, and
// one application of   A x = S (A_box x_box - sum_{refined box cells c} K_c x_box) + sum_{fine cells f} K_f x,   x_box = S^T x   (kernels_hyb.hip).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <unordered_map>
#include "common.hpp"
#include "ctx_internal.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace poro {
namespace ctx_detail {
namespace {

template <class T> std::vector<T> download(const DevBuf<T> &b) {
  std::vector<T> h(b.n);
  if (b.n) PORO_HIP(hipMemcpy(h.data(), b.p, b.n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

// the plan, from the interpolation rows, the two cell lists, the vertices and the Dirichlet masks.  Throws (and leaves `H` unbuilt) where the mesh is not a box
// with some cells split once, lying exactly on the coarse box
void derive_plan(poro_ctx *c, HybridPlan &H) {
  poro_ctx *B = c->two_level.box; const int dim = c->dim, nv = c->nv, dpc = c->dpc_u;
  const int64_t nb = B->n_u / dim, nm = c->n_u / dim, ncb = B->n_cells, ncm = c->n_cells;
  PORO_HIP(hipStreamSynchronize(c->stream));
  if (c->mat.lame_lambda != B->mat.lame_lambda || c->mat.shear_G != B->mat.shear_G) throw Error("hybrid operator: the material constants of the mesh and of its coarse box differ");

  // injection: box node b <-> the one mesh node whose interpolation row is the single entry (b, 1.0)
  std::vector<int64_t> inj((size_t)nb, -1);
  { const std::vector<int64_t> ptr = download(c->two_level.p_ptr); const std::vector<int32_t> col = download(c->two_level.p_col); const std::vector<double> w = download(c->two_level.p_w);
    if ((int64_t)ptr.size() != nm + 1 || c->two_level.n_coarse != nb) throw Error("hybrid operator: the interpolation rows do not belong to this mesh and its coarse box");
    for (int64_t i = 0; i < nm; ++i) {
      if (ptr[i + 1] - ptr[i] != 1 || w[ptr[i]] != 1.0) continue;
      const int32_t b = col[ptr[i]];
      if (inj[b] >= 0) throw Error("hybrid operator: box node " + std::to_string(b) + " is the image of two mesh nodes");
      inj[b] = i;
    }
    for (int64_t b = 0; b < nb; ++b) if (inj[b] < 0) throw Error("hybrid operator: box node " + std::to_string(b) + " has no injected image among the mesh nodes (the mesh is not a refinement of its coarse box, e.g. an auxiliary box)"); }

  // unrefined cells: the dof list is, entry by entry, the injected dof list of a box cell
  const std::vector<int32_t> cdm = download(c->cell_dofs_u), cdb = download(B->cell_dofs_u);
  std::unordered_map<int64_t, int64_t> first;      // injected first dof -> box cell
  first.reserve((size_t)ncb * 2);
  auto injected = [&](int32_t box_dof) { return inj[box_dof / dim] * dim + box_dof % dim; };
  for (int64_t k = 0; k < ncb; ++k) first.emplace(injected(cdb[(size_t)k * dpc]), k);
  std::vector<int64_t> twin((size_t)ncm, -1);      // mesh cell -> matched box cell
  std::vector<uint8_t> removed((size_t)ncb, 1);
  for (int64_t e = 0; e < ncm; ++e) {
    const auto it = first.find(cdm[(size_t)e * dpc]);
    if (it == first.end()) continue;
    const int64_t k = it->second; bool same = true;
    for (int j = 0; j < dpc && same; ++j) same = injected(cdb[(size_t)k * dpc + j]) == cdm[(size_t)e * dpc + j];
    if (same) { if (!removed[k]) throw Error("hybrid operator: two mesh cells match box cell " + std::to_string(k)); twin[e] = k; removed[k] = 0; }
  }
  int64_t n_removed = 0, n_fine = 0;
  for (int64_t k = 0; k < ncb; ++k) n_removed += removed[k];
  for (int64_t e = 0; e < ncm; ++e) n_fine += twin[e] < 0;
  if (n_fine != n_removed * (int64_t)(1 << dim))
    throw Error("hybrid operator: unmatched cells (" + std::to_string(n_fine) + " mesh cells match no box cell, " + std::to_string(n_removed) + " box cells are matched by none: not 2^dim children each)");

  // geometry: matched cells lie on their box cells; every fine cell has its centroid inside a refined box cell, 2^dim of them in each
  { const std::vector<double> Xm = download(c->cell_X), Xb = download(B->cell_X);
    double lo[3] = {0, 0, 0}, extent = 0;
    for (int d = 0; d < dim; ++d) { lo[d] = Xb[d]; extent = std::max(extent, B->box.n[d] * B->box.h[d]); }
    const double tol = 1e-12 * extent;
    std::vector<int32_t> children((size_t)ncb, 0);
    for (int64_t e = 0; e < ncm; ++e) {
      const double *x = Xm.data() + (size_t)e * nv * dim;
      if (twin[e] >= 0) {
        const double *xb = Xb.data() + (size_t)twin[e] * nv * dim;
        for (int i = 0; i < nv * dim; ++i) if (!(std::fabs(x[i] - xb[i]) <= tol))
          throw Error("hybrid operator: the vertices of mesh cell " + std::to_string(e) + " differ from those of its box cell by more than 1e-12 of the box extent (a mapped mesh: its unrefined cells are not the box's congruent cells)");
        continue;
      }
      int64_t k = 0, stride = 1; bool inside = true;
      for (int d = 0; d < dim; ++d) {
        double m = 0; for (int v = 0; v < nv; ++v) m += x[v * dim + d];
        const double t = (m / nv - lo[d]) / B->box.h[d]; const int64_t i = (int64_t)std::floor(t);
        if (!(t >= 0) || i >= B->box.n[d]) { inside = false; break; }
        k += i * stride; stride *= B->box.n[d];
      }
      if (!inside || !removed[k]) throw Error("hybrid operator: unmatched cells (the centroid of mesh cell " + std::to_string(e) + " lies in no refined box cell)");
      children[k]++;
    }
    for (int64_t k = 0; k < ncb; ++k) if (removed[k] && children[k] != (1 << dim)) throw Error("hybrid operator: unmatched cells (refined box cell " + std::to_string(k) + " holds " + std::to_string(children[k]) + " fine cells, not 2^dim)"); }

  // Dirichlet data: the box product zeroes the box's Dirichlet columns, the fine cells the mesh's
  { const std::vector<uint8_t> mm = download(c->dir_mask), mb = download(B->dir_mask);
    for (int64_t b = 0; b < nb; ++b) for (int a = 0; a < dim; ++a)
      if ((mm[inj[b] * dim + a] != 0) != (mb[b * dim + a] != 0)) throw Error("hybrid operator: the Dirichlet mask of the mesh differs from the coarse box's at box node " + std::to_string(b)); }

  // the fine cells in the context's colour classes and in the Morton order of the atomic mode
  { const std::vector<int32_t> cc = download(c->color_cells); std::vector<int32_t> fine; fine.reserve((size_t)n_fine);
    H.color_off.assign(1, 0);
    for (size_t q = 0; q + 1 < c->color_off.size(); ++q) {
      for (int64_t i = c->color_off[q]; i < c->color_off[q + 1]; ++i) if (twin[cc[i]] < 0) fine.push_back(cc[i]);
      H.color_off.push_back((int64_t)fine.size());
    }
    H.color_cells.upload(fine);
    build_spatial_cells(c);
    const std::vector<int32_t> sc = download(c->spatial_cells); fine.clear();
    for (int32_t e : sc) if (twin[e] < 0) fine.push_back(e);
    H.spatial_cells.upload(fine); }

  // box nodes of the refined cells, sorted by position class (Q2: bit d = mid node in direction d), every class padded to whole waves
  { std::vector<uint8_t> touched((size_t)nb, 0);
    for (int64_t k = 0; k < ncb; ++k) if (removed[k]) for (int j = 0; j < dpc; j += dim) touched[cdb[(size_t)k * dpc + j] / dim] = 1;
    const int n_cls = c->k_u == 2 ? 1 << dim : 1; const int64_t nn0 = B->box.nn[0], nn1 = B->box.nn[1];
    std::vector<std::vector<int64_t>> by_cls((size_t)n_cls);
    for (int64_t b = 0; b < nb; ++b) if (touched[b]) {
      const int64_t i[3] = {b % nn0, (b / nn0) % nn1, b / (nn0 * nn1)};
      int cls = 0; if (c->k_u == 2) for (int d = 0; d < dim; ++d) cls |= (int)(i[d] & 1) << d;
      by_cls[cls].push_back(b);
    }
    std::vector<int64_t> nodes; std::vector<int32_t> chunk_cls;
    for (int q = 0; q < n_cls; ++q) {
      nodes.insert(nodes.end(), by_cls[q].begin(), by_cls[q].end());
      while (nodes.size() % 64) nodes.push_back(-1);
      chunk_cls.resize(nodes.size() / 64, q);
    }
    H.n_chunks = (int64_t)chunk_cls.size();
    std::vector<int32_t> cells, slot((size_t)ncb, -1);
    for (int64_t k = 0; k < ncb; ++k) if (removed[k]) { slot[k] = (int32_t)cells.size(); cells.push_back((int32_t)k); }
    H.nodes.upload(nodes); H.chunk_cls.upload(chunk_cls); H.touched.upload(touched); H.removed_cells.upload(cells); H.slot.upload(slot);
    H.V.alloc((size_t)n_removed * dpc); H.V.zero(c->stream); }

  H.inj.upload(inj);
  H.x_box.alloc(B->n_u); H.y_box.alloc(B->n_u); H.x_box.zero(c->stream); H.y_box.zero(c->stream);
  H.n_box_nodes = nb; H.n_fine_cells = n_fine; H.n_removed = n_removed;
  // the box context's element matrix: assembled by its poro_disp_assemble_system, which nobody may have called (the two-level preconditioner does not need it)
  if (!B->Ke.p) B->Ke.alloc((size_t)B->dpc_u * B->dpc_u);
  asm_u_element_matrix(c->stream, asm_args(B), 0, B->Ke.p);
  PORO_HIP(hipStreamSynchronize(c->stream));
  { const std::vector<double> ke = download(B->Ke); std::vector<double> kt(ke.size());      // the transposed copy the refined-cell kernel walks (coalesced over the rows)
    for (int i = 0; i < dpc; ++i) for (int j = 0; j < dpc; ++j) kt[(size_t)j * dpc + i] = ke[(size_t)i * dpc + j];
    H.Ke_t.upload(kt); }
}

void apply_with(poro_ctx *c, const HybridPlan &H, const double *x, double *y, bool constrained, bool count) {
  hipStream_t s = c->stream; poro_ctx *B = c->two_level.box;
  // fine cells (this zeroes y); no fine cell: the memset alone
  const int32_t *all = c->scatter_mode == PORO_SCATTER_ATOMIC ? H.spatial_cells.p : nullptr;
  const int launches = mfg_apply(s, asm_args(c), H.color_cells.p, H.color_off, c->n_u, x, y, constrained, 0, all);
  if (count) count_mfg_launches(c, launches);
  Timed tm(c, "apply_u_hybrid_box");
  const MfArgs box = mf_args(B);
  hyb_gather(s, c->dim, H.n_box_nodes, H.inj.p, x, H.x_box.p);
  kron_apply(s, box, H.x_box.p, H.y_box.p, constrained, c->n_cus);
  const HybCombine h{H.n_box_nodes, H.n_removed, H.n_chunks, H.inj.p, H.touched.p, H.removed_cells.p, H.slot.p, H.chunk_cls.p, H.nodes.p, H.x_box.p, H.y_box.p, H.V.p};
  hyb_combine(s, box, H.Ke_t.p, constrained, h, y);
}

}  // namespace

void hybrid_enable(poro_ctx *c) {
  if (!c->two_level.box) throw Error("hybrid operator: the context has no coarse space (poro_desc.coarse: the underlying uniform box of a refined box)");
  if (c->comm.multi()) throw Error("hybrid operator: not on partitioned contexts (one rank only)");
  if (c->operator_mode != PORO_OP_MATRIX_FREE) throw Error("hybrid operator: the context was not created with PORO_OP_MATRIX_FREE");
  if (!kron_supported(c->dim, c->k_u)) throw Error("hybrid operator: no structured kernel for this dimension / degree");
  if (c->hyb.built) return;
  HybridPlan &H = c->hyb;
  try {
    derive_plan(c, H);
    if (!std::getenv("PORO_DIAG_SKIP_SELFCHECK")) {
      // one hybrid product of a fixed pseudo-random vector against the general coloured product over all cells, both with their Dirichlet rows fixed as by mf_operator
      // (the cell kernels leave those rows zero, the structured kernel does not)
      std::vector<double> hx((size_t)c->n_u), y1((size_t)c->n_u), y2((size_t)c->n_u);
      uint64_t r = 0x9e3779b97f4a7c15ull;
      for (double &v : hx) { r = r * 6364136223846793005ull + 1442695040888963407ull; v = (double)(r >> 11) / 9007199254740992.0 - 0.5; }
      DevBuf<double> x, y; x.upload(hx); y.alloc(c->n_u);
      const int saved = c->scatter_mode; c->scatter_mode = PORO_SCATTER_COLOURED;
      try { apply_with(c, H, x.p, y.p, true, false); } catch (...) { c->scatter_mode = saved; throw; }
      c->scatter_mode = saved;
      kron_fix_constrained(c->stream, mf_args(c), x.p, y.p, nullptr, 0);
      PORO_HIP(hipMemcpyAsync(y1.data(), y.p, y1.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      mfg_apply(c->stream, asm_args(c), c->color_cells.p, c->color_off, c->n_u, x.p, y.p, true, 0);
      kron_fix_constrained(c->stream, mf_args(c), x.p, y.p, nullptr, 0);
      PORO_HIP(hipMemcpyAsync(y2.data(), y.p, y2.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      PORO_HIP(hipStreamSynchronize(c->stream));
      double diff = 0, top = 0;
      for (size_t i = 0; i < y1.size(); ++i) { diff = std::max(diff, std::fabs(y1[i] - y2[i])); top = std::max(top, std::fabs(y2[i])); }
      if (!(diff <= 1e-11 * top)) throw Error("hybrid operator disagrees with the general cell loop: max diff " + std::to_string(diff) + " vs max " + std::to_string(top));
    }
    H.built = true;
  } catch (...) {
    H.inj.release(); H.color_cells.release(); H.spatial_cells.release(); H.removed_cells.release(); H.slot.release(); H.Ke_t.release(); H.V.release(); H.touched.release(); H.nodes.release(); H.chunk_cls.release(); H.x_box.release(); H.y_box.release();
    H.color_off.clear(); H.n_box_nodes = H.n_fine_cells = H.n_removed = H.n_chunks = 0;
    throw;
  }
}

void hybrid_operator(poro_ctx *c, const double *x, double *y, bool constrained) { apply_with(c, c->hyb, x, y, constrained, true); }

}  // namespace ctx_detail
}  // namespace poro
