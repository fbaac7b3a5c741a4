// Mesh adaptation entry points (refine_mesh, PoroelasticityFSS.h:447-498): the face tables and the driver of the Kelly error indicator, and the transfer of the three
// pressure-space vectors between two contexts.  The kernels are in kernels_kelly.hip.
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <map>
#include "common.hpp"
#include "ctx_internal.hpp"
#include "kelly_tables.hpp"

using namespace poro;
using namespace poro::ctx_detail;

namespace poro {
namespace ctx_detail {

// CSR-like rows handed in by a caller: checked on the host before anything is uploaded or walked (ptr[0] == 0, ascending, column indices in range)
void validate_rows(const int64_t *ptr, const int32_t *col, const double *weight, int64_t n_rows, int64_t n_cols, const std::string &what) {
  if (n_rows < 0 || !ptr) throw Error(what + ": row offsets missing");
  if (ptr[0] != 0) throw Error(what + ": ptr[0] must be 0");
  for (int64_t i = 0; i < n_rows; ++i) if (ptr[i + 1] < ptr[i]) throw Error(what + ": ptr not monotone");
  const int64_t nnz = ptr[n_rows];
  if (nnz && (!col || !weight)) throw Error(what + ": node / weight missing");
  for (int64_t k = 0; k < nnz; ++k) if (col[k] < 0 || col[k] >= n_cols) throw Error(what + ": node out of range");
}

namespace {
template <class T> std::vector<T> download(const DevBuf<T> &b, size_t n) {
  std::vector<T> h(n);
  if (n) { if (!b.p || b.n < n) throw Error("kelly: a mesh array is missing on the device"); PORO_HIP(hipMemcpy(h.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost)); }
  return h;
}
}  // namespace

// the face tables (kelly_tables.hpp) from the mesh arrays the context keeps on the device; built once
void build_kelly_tables(poro_ctx *c) {
  KellyDev &K = c->kelly;
  if (K.built) return;
  const int nv = c->nv; const int64_t nc = c->n_cells;
  PORO_HIP(hipStreamSynchronize(c->stream));
  const std::vector<int32_t> cv = download(c->cell_dofs_p, (size_t)nc * nv);
  const std::vector<int32_t> bfc = download(c->bface_cell, (size_t)c->n_bfaces), bfl = download(c->bface_local, (size_t)c->n_bfaces);
  const int64_t n_cons = c->cons_p.n;
  std::vector<int32_t> hdof, hmaster; std::vector<int64_t> hptr(1, 0); std::vector<double> hw;
  if (n_cons) {
    hdof = download(c->cons_p.dof, (size_t)n_cons); hptr = download(c->cons_p.ptr, (size_t)n_cons + 1);
    hmaster = download(c->cons_p.master, (size_t)hptr[n_cons]); hw = download(c->cons_p.weight, (size_t)hptr[n_cons]);
  }
  const KellyTables T = build_kelly_tables_host(c->dim, nc, c->n_p, cv, c->n_bfaces, bfc, bfl, n_cons, hdof, hptr, hmaster, hw);
  K.n_faces = (int64_t)T.cell_a.size();
  K.cell_a.upload(T.cell_a); K.cell_b.upload(T.cell_b); K.code.upload(T.code); K.ent_ptr.upload(T.ent_ptr); K.ent_face.upload(T.ent_face); K.ent_hcell.upload(T.ent_hcell);
  K.jump.alloc((size_t)K.n_faces); K.eta.alloc((size_t)nc);
  K.built = true;
}

}  // namespace ctx_detail
}  // namespace poro

namespace {
bool pressure_space_vector(poro_ctx *c, int which) {
  auto it = c->vec.find(which);
  if (it == c->vec.end()) throw Error("unknown vector id " + std::to_string(which));
  return !is_u_vec(which) && (int64_t)it->second.n == c->n_p;
}
}  // namespace

extern "C" {

int poro_pres_estimate_error(poro_ctx *c, int which_vec, double *eta_host) {
  return guarded([&] {
    if (!c || !eta_host) throw Error("null argument");
    if (c->comm.part.n_ranks > 1) throw Error("poro_pres_estimate_error: not implemented on partitioned contexts (n_ranks > 1): the faces between ranks are not known to a rank");
    if (!pressure_space_vector(c, which_vec)) throw Error("poro_pres_estimate_error: vector " + std::to_string(which_vec) + " is not a pressure-space vector");
    PORO_HIP(hipSetDevice(c->device));
    build_kelly_tables(c);
    KellyDev &K = c->kelly;
    { Timed tm(c, "kelly");
      kelly_faces(c->stream, c->dim, K.n_faces, K.cell_a.p, K.cell_b.p, K.code.p, c->cell_X.p, c->cell_dofs_p.p, vec(c, which_vec), K.jump.p);
      kelly_cells(c->stream, c->dim, c->n_cells, K.ent_ptr.p, K.ent_face.p, K.ent_hcell.p, c->cell_X.p, K.jump.p, K.eta.p); }
    PORO_HIP(hipMemcpyAsync(eta_host, K.eta.p, (size_t)c->n_cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PORO_HIP(hipStreamSynchronize(c->stream));
    return 0;
  });
}

int poro_state_transfer_p(poro_ctx *from, poro_ctx *to, const int64_t *ptr, const int32_t *node, const double *weight) {
  return guarded([&] {
    if (!from || !to) throw Error("null argument");
    if (from == to) throw Error("poro_state_transfer_p: `from` and `to` are the same context");
    if (from->device != to->device) throw Error("poro_state_transfer_p: the two contexts are on different devices");
    if (from->comm.part.n_ranks > 1 || to->comm.part.n_ranks > 1) throw Error("poro_state_transfer_p: not implemented on partitioned contexts (n_ranks > 1)");
    validate_rows(ptr, node, weight, to->n_p, from->n_p, "poro_state_transfer_p");
    PORO_HIP(hipSetDevice(to->device));
    DevBuf<int64_t> dptr; DevBuf<int32_t> dnode; DevBuf<double> dw;
    dptr.upload(ptr, (size_t)to->n_p + 1); dnode.upload(node, (size_t)ptr[to->n_p]); dw.upload(weight, (size_t)ptr[to->n_p]);
    static const int ids[3] = {PORO_VEC_P, PORO_VEC_EPSV, PORO_VEC_EPSV0};
    const double *in[3]; double *out[3];
    for (int e = 0; e < 3; ++e) { in[e] = vec(from, ids[e]); out[e] = vec(to, ids[e]); }
    // after everything `from` has enqueued, on `to`'s stream
    hipEvent_t ev = nullptr; PORO_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e1 = hipEventRecord(ev, from->stream), e2 = e1 == hipSuccess ? hipStreamWaitEvent(to->stream, ev, 0) : e1;
    if (e2 == hipSuccess) { Timed tm(to, "transfer_p"); transfer_rows3(to->stream, to->n_p, dptr.p, dnode.p, dw.p, in, out); }
    const hipError_t e3 = e2 == hipSuccess ? hipStreamSynchronize(to->stream) : e2;   // the rows are freed on return, and `from` may be destroyed right after
    (void)hipEventDestroy(ev);
    PORO_HIP(e3);
    return 0;
  });
}

}  // extern "C"
