// Octant form of the block fast-diagonalisation preconditioner of the displacement system (K-prec; the preconditioner slot of
// PoroElasticDisplacementSolver<dim>::solve, PoroElasticDisplacementSolver.h:302-305) on 3D uniform boxes, one rank (gfx950, wave64, fp64 MFMA).
//
// kernels_fdmu.hip exploits that on a mirror-symmetric line every generalised eigenvector of the 1D FE_Q(k) pencil is even or odd: with
// e_k = v_k + v_k', o_k = v_k - v_k' (k < h = (n + 1) / 2, k' = n - 1 - k; the centre node of an odd line is its own mirror: e = v, o = 0) a 1D
// transform splits into two half-size products.  There the butterflies run inside every transform pass, and the passes still read / write the
// node-interleaved CG vectors (24-byte strides: 2.4 x the useful HBM traffic in the x passes, profiles/r03_fdmu_baseline_counters.txt).  Here the
// butterflies of all three directions are hoisted OUT of the preconditioner: they commute with the 1D transforms of the other directions, so
//     z = H' (sum over the 8 parity octants of independent half-size 3D fast diagonalisations) H g,
// with H the 8-point butterfly.  The CG residual g and z = P^-1 g therefore LIVE in octant form Q[c][o][kz][ky][kx] (o = 4 pz + 2 py + px), and H / H'
// ride in the CG update kernels, which touch every entry anyway (g += alpha A d reads the eight mirror images of A d; d = -z + beta d scatters to them;
// g.z = sum Q_g Q_z and |g|^2 = weighted sum Q_g^2 hold in octant form directly).  What is left of the preconditioner is 24 independent
// (component, octant) blocks of h^3 entries, each a plain 3D tensor transform in contiguous planar storage:
//     pass 1  (x, y fused per z-plane)    X[ky][kx] -> Fy X Fx^T
//     pass 2  (z; per 16 NT columns)      X[kz][col] -> Bz diag(1 / (kx lam_x + ky lam_y + kz lam_z)) Fz X        (in place)
//     pass 3  (y, x fused per z-plane)    X[my][mx] -> By X Bx^T
// = 3 sweeps over the vector instead of 5, every access contiguous.  All three passes are ONE kernel: a block of <= 80 x 80 doubles is staged
// in LDS, two chained GEMMs on v_mfma_f64_16x16x4_f64 with the data passing through LDS between them (in the bank-conflict-free layout the second
// GEMM's operand reads need), the half-size transform matrices as the other operand straight from L2 in MFMA fragment order (each wave only needs
// the 16 rows of its own output tile).  "contract columns": Y = X T^T, wave w owns output column tile w, data = A operand; "contract rows":
// Y = T X, wave s owns output row tile s, data = B operand; either way the accumulator of tile (T, W) holds element (16 T + 4 q + kq, 16 W + j) in
// register q of lane j + 16 kq, so one store routine serves both.
//
// Per-direction form (opt-in, poro_ctx_set_fdm_form): the same three passes on boxes where only SOME directions are mirror-symmetric (one-sided Dirichlet faces, graded lines).  A
// direction that is split keeps the above; a WHOLE direction has no butterfly and a whole-length transform: 2^(split directions) parity parts per component instead of eight, and
// per-pass tile counts (passes 1 / 3: max(len_x, len_y), pass 2: len_z).  OctDims carries the split mask for the vector kernels, k_fdmo_pass has VAR = 3 for the passes.
#include "common.hpp"
#include "fdm_tables.hpp"
#include "device_reduce.hpp"
#include <hip/hip_ext.h>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <set>
#include <type_traits>

namespace poro {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct OctDims { int nx, ny, nz, hx, hy, hz, hxp; int64_t co; int no, own_z, nc; int split; int part[8]; };   // nodes and half lengths per direction; hxp = row pitch (hx rounded up to even: 16-byte aligned rows, the pad entry stays zero); co = hxp hy hz entries per (component, octant)
// (per-direction form, PD instantiations of the vector kernels) split: bit d set = direction d is split in parities (mirror index n - 1 - k); clear = whole: every index is "its own mirror image" (h = n, no butterfly).  no = parity parts per
// component = 2^(split directions); part[o] = block of parity combination o = 4 pz + 2 py + px inside a component (the bits of the split directions, packed), -1 where o has a bit of
// a whole direction.  7: octant form (part[o] = o); 3 (slab partitions, planar form): quadrants; 0: the plain nodal values in planar storage; own_z = planes that count in dot products

// ---- the 8-point butterfly --------------------------------------------------------------------------------------------------------------
// index bit 0 / 1 / 2 = x / y / z.  Forward: in = values at the lower node (bit clear) and its mirror image (bit set), out = even (bit clear) and odd
// (bit set) parts; a direction whose lower index is the centre of an odd line has no mirror: even = the value, odd = 0.
__device__ __forceinline__ void bfly_fwd(double (&v)[8], const bool (&centre)[3]) {
#pragma unroll
  for (int bit = 0; bit < 3; ++bit) {
    const int m = 1 << bit;
#pragma unroll
    for (int i = 0; i < 8; ++i) if (!(i & m)) {
      const double lo = v[i], hi = v[i | m];
      v[i] = centre[bit] ? lo : lo + hi; v[i | m] = centre[bit] ? 0.0 : lo - hi;
    }
  }
}
// Backward: in = the even-mode / odd-mode partial sums (a, b), out = node values v_k = a + b, v_k' = a - b (centre: v = a, the mirror slot is unused)
__device__ __forceinline__ void bfly_bwd(double (&v)[8], const bool (&centre)[3]) {
#pragma unroll
  for (int bit = 0; bit < 3; ++bit) {
    const int m = 1 << bit;
#pragma unroll
    for (int i = 0; i < 8; ++i) if (!(i & m)) {
      const double a = v[i], b = v[i | m];
      v[i] = centre[bit] ? a : a + b; v[i | m] = centre[bit] ? a : a - b;
    }
  }
}
// PD (per-direction form): mirrors and the blocks of the parts from D.split / D.part.  PD = false (octants, quadrants, no split) derives them from D.no as always, so that the
// kernels of the existing forms compile to what they were
template <bool PD> __device__ __forceinline__ bool part_on(const OctDims &D, int o) { return PD ? D.part[o] >= 0 : o < D.no; }
template <bool PD> __device__ __forceinline__ int part_at(const OctDims &D, int o) { return PD ? D.part[o] : o; }
template <bool PD> struct OctPos {
  int64_t node[8]; bool centre[3]; bool live[8]; double weight; bool valid, own;
  // lower-octant position idx = (kz hy + ky) hxp + kx -> the eight mirror nodes; live[m]: node m is distinct from the ones with fewer mirrored directions; valid: not a row pad
  __device__ __forceinline__ OctPos(const OctDims &D, int64_t idx) {
    const int kx = (int)(idx % D.hxp), ky = (int)((idx / D.hxp) % D.hy), kz = (int)(idx / ((int64_t)D.hxp * D.hy));
    valid = kx < D.hx;
    const int mx = PD ? ((D.split & 1) ? D.nx - 1 - kx : kx) : (D.no == 1 ? kx : D.nx - 1 - kx), my = PD ? ((D.split & 2) ? D.ny - 1 - ky : ky) : (D.no == 1 ? ky : D.ny - 1 - ky),
              mz = PD ? ((D.split & 4) ? D.nz - 1 - kz : kz) : (D.no == 8 ? D.nz - 1 - kz : kz);   // (PD = false: no = 8 octants, 4: z not split, 1: no direction is split - the plain nodal values in planar storage)
    centre[0] = mx == kx; centre[1] = my == ky; centre[2] = mz == kz; own = kz < D.own_z;
    weight = (centre[0] ? 1.0 : 0.5) * (centre[1] ? 1.0 : 0.5) * (centre[2] ? 1.0 : 0.5);   // |v|^2 over a mirror orbit = weight * sum of the squared parity parts
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int x = (m & 1) ? mx : kx, y = (m & 2) ? my : ky, z = (m & 4) ? mz : kz;
      node[m] = ((int64_t)z * D.ny + y) * D.nx + x;
      live[m] = !((m & 1) && centre[0]) && !((m & 2) && centre[1]) && !((m & 4) && centre[2]);
    }
  }
};

// Thread mapping of the vector kernels: thread t <-> (lower-octant position t / 3, component t % 3), so that the lanes of a wave walk through the node-interleaved
// vectors contiguously (dof = 3 node + c: 512 contiguous bytes per wave access, ascending for the lower nodes, descending for the mirror images) and through three
// contiguous streams of every octant array.  (First version: one thread per position, all three components - 8-byte accesses at 24-byte stride: 170 us for the
// direction update instead of 45.)
#define PORO_OCT_LOOP(D) for (int64_t t_ = (int64_t)blockIdx.x * kBlock + threadIdx.x; t_ < NC * (D).co; t_ += (int64_t)gridDim.x * kBlock)   /* NC = components per node: 3, or 2 for the planar form */
#define PORO_OCT_DECODE(D) const int64_t idx = t_ / NC; const int c = (int)(t_ - NC * idx); const OctPos<PD> P(D, idx); if (!P.valid) continue;

// q = H v: node-interleaved vector (dof = 3 node + c) -> octant form; masked dofs count as zero
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_from_nodal(OctDims D, const double *__restrict__ v, const uint8_t *__restrict__ inert, double *__restrict__ q) {
  PORO_OCT_LOOP(D) {
    PORO_OCT_DECODE(D)
    double w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) { const int64_t dof = P.node[m] * NC + c; w[m] = (inert && inert[dof]) ? 0.0 : v[dof]; }
    bfly_fwd(w, P.centre);
#pragma unroll
    for (int o = 0; o < 8; ++o) if (part_on<PD>(D, o)) q[(int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx] = w[o];
  }
}
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_to_nodal(OctDims D, const double *__restrict__ r, double *__restrict__ v) {
  PORO_OCT_LOOP(D) {
    PORO_OCT_DECODE(D)
    double w[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) w[o] = part_on<PD>(D, o) ? r[(int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx] : 0.0;
    bfly_bwd(w, P.centre);
#pragma unroll
    for (int m = 0; m < 8; ++m) if (P.live[m]) v[P.node[m] * NC + c] = w[m];
  }
}

// ---- CG vector kernels with g, z in octant form (protocol of k_pcg_* in kernels_la.hip) ---------------------------------------------------
// g = H (A x - b), zero on the inert (Dirichlet) dofs
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_init_residual(OctDims D, double *__restrict__ g, const double *__restrict__ Ax, const double *__restrict__ b, const uint8_t *__restrict__ inert) {
  PORO_OCT_LOOP(D) {
    PORO_OCT_DECODE(D)
    double w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) { const int64_t dof = P.node[m] * NC + c; w[m] = (inert && inert[dof]) ? 0.0 : Ax[dof] - b[dof]; }
    bfly_fwd(w, P.centre);
#pragma unroll
    for (int o = 0; o < 8; ++o) if (part_on<PD>(D, o)) g[(int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx] = w[o];
  }
}
// d = -z (nodal); block partials of g.g and g.z
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_first_direction(OctDims D, double *__restrict__ d, const double *__restrict__ g, const double *__restrict__ z, double *partials) {
  __shared__ double sh[5];
  double gg = 0, gz = 0;
  PORO_OCT_LOOP(D) {
    PORO_OCT_DECODE(D)
    double w[8]; double s2 = 0, sz = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) { w[o] = 0.0; if (part_on<PD>(D, o)) { const int64_t at = (int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx; const double gv = g[at]; w[o] = z[at]; s2 = fma(gv, gv, s2); sz = fma(gv, w[o], sz); } }
    if (P.own) { gg = fma(P.weight, s2, gg); gz += sz; }
    bfly_bwd(w, P.centre);
#pragma unroll
    for (int m = 0; m < 8; ++m) if (P.live[m]) d[P.node[m] * NC + c] = -w[m];
  }
  gg = block_sum(gg, sh); gz = block_sum(gz, sh);
  store_partial(partials, gg); store_partial(partials + kMaxPartials, gz);
}
// g += alpha H (A d) and the partials of g.g (g.z follows in a plain dot of the two octant arrays once z = P^-1 g exists)
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_update_g(OctDims D, PcgScalars *sc, int parity, double *__restrict__ g, const double *__restrict__ h, const uint8_t *__restrict__ inert, const double *partials_dh, double *partials_out, const double *red) {
  __shared__ double sh[5];
  if (sc->done) return;
  if (sc->finishing) { if (blockIdx.x == 0 && threadIdx.x == 0) sc->done = 1; return; }   // (see k_pcg_update_g_fused)
  const double dh = red ? red[0] : sum_partials(partials_dh, sh);
  const double alpha = sc->gh2[parity] / dh;
  double gg = 0;
  PORO_OCT_LOOP(D) {
    PORO_OCT_DECODE(D)
    // inert (Dirichlet) dofs: the residual stays exactly zero whatever the operator left in h.  The octant form exists only where every Dirichlet condition covers a
    // pair of opposite faces (build_fdm_u), so the eight mirror images of a dof are inert together: one mask byte per thread.  (Per-direction form: a direction is split only
    // where every component has the same condition at both of its ends, and a whole direction has no mirror image - the same holds)
    if (inert && inert[P.node[0] * NC + c]) continue;
    double w[8]; double s2 = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) w[m] = h[P.node[m] * NC + c];
    bfly_fwd(w, P.centre);
#pragma unroll
    for (int o = 0; o < 8; ++o) if (part_on<PD>(D, o)) { const int64_t at = (int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx; const double gv = fma(alpha, w[o], g[at]); g[at] = gv; s2 = fma(gv, gv, s2); }
    if (P.own) gg = fma(P.weight, s2, gg);
  }
  gg = block_sum(gg, sh);
  store_partial(partials_out, gg);
  if (blockIdx.x == 0 && threadIdx.x == 0) { sc->dh = dh; sc->alpha = alpha; }
}
// the same with TWO neighbouring positions (idx, idx + 1: same row, the pitch is even) per thread: 16-byte accesses on the octant side (twice as long contiguous pieces per
// component and instruction), the nodal side reads two dofs 8 NC bytes apart
template <int NC, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_update_g2(OctDims D, PcgScalars *sc, int parity, double *__restrict__ g, const double *__restrict__ h, const uint8_t *__restrict__ inert, const double *partials_dh, double *partials_out, const double *red) {
  __shared__ double sh[5];
  if (sc->done) return;
  if (sc->finishing) { if (blockIdx.x == 0 && threadIdx.x == 0) sc->done = 1; return; }
  const double dh = red ? red[0] : sum_partials(partials_dh, sh);
  const double alpha = sc->gh2[parity] / dh;
  double gg = 0;
  for (int64_t t_ = (int64_t)blockIdx.x * kBlock + threadIdx.x; t_ < NC * (D.co / 2); t_ += (int64_t)gridDim.x * kBlock) {
    const int64_t pr = t_ / NC; const int c = (int)(t_ - NC * pr); const int64_t idx = 2 * pr;
    const OctPos<PD> P0(D, idx), P1(D, idx + 1);
    double w0[8], w1[8];
    const bool on0 = P0.valid && !(inert && inert[P0.node[0] * NC + c]), on1 = P1.valid && !(inert && inert[P1.node[0] * NC + c]);
#pragma unroll
    for (int m = 0; m < 8; ++m) { w0[m] = on0 ? h[P0.node[m] * NC + c] : 0.0; w1[m] = on1 ? h[P1.node[m] * NC + c] : 0.0; }
    bfly_fwd(w0, P0.centre); bfly_fwd(w1, P1.centre);
    double s0 = 0, s1 = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) if (part_on<PD>(D, o)) {
      double2 *gp = reinterpret_cast<double2 *>(g + (int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx);
      double2 gv = *gp;
      gv.x = fma(alpha, w0[o], gv.x); gv.y = fma(alpha, w1[o], gv.y);       // (inert dofs and row pads: w = 0, g stays what it is - zero)
      *gp = gv; s0 = fma(gv.x, gv.x, s0); s1 = fma(gv.y, gv.y, s1);
    }
    if (P0.own) gg = fma(P0.weight, s0, fma(P1.weight, s1, gg));
  }
  gg = block_sum(gg, sh);
  store_partial(partials_out, gg);
  if (blockIdx.x == 0 && threadIdx.x == 0) { sc->dh = dh; sc->alpha = alpha; }
}
// x += alpha d, then d = beta d - H' z unless the solve just finished (k_pcg_update_d_fused with the explicit z in octant form)
// g . z: the gz_n per-workgroup partials of transform pass 2 (gz_part != null), else the second set of partials_in (separate dot kernel)
// XNT: x is touched once per iteration and nowhere else: non-temporal accesses keep it from evicting d, g and the shared h | z array (224.6 MB at 72^3 Q2), which then
// stay in the 256 MiB memory-side cache from one kernel of the iteration to the next (as in k_pcg_update_d_fused).  d and z keep plain accesses, and so does the
// finishing branch below on purpose: it runs once per solve, after the last use of d, g and z.
template <int NC, bool XNT, bool PD> __global__ void __launch_bounds__(kBlock) k_fdmo_update_d(OctDims D, PcgScalars *sc, int parity, int it, double *__restrict__ x, double *__restrict__ d, const double *__restrict__ z, int64_t n_u, const double *partials_in, const double *red,
                                                                            const double *gz_part, int gz_n, int decided /* 2: and sc->gg holds g . g */) {
  __shared__ double sh[5];
  if (sc->done) return;
  // decided: the stopping test of this iteration ran in front of the preconditioner call (PcgStopTest) and sc->stop holds its outcome - taken as it stands, never tested
  // again: when it finished the solve, no kernel of the call has run, z and the g . z partials are stale and are neither read nor recorded
  // decided == 2: workgroup 0 of the kernel that ran the test stored the sum it tested (the same partials in the same order: the same bits) - one word instead of 8 KB and four barriers
  const double gg = red ? red[0] : decided == 2 ? sc->gg : sum_partials(partials_in, sh);
  const double res = sqrt(gg), gh_old = sc->gh2[parity], alpha = sc->alpha;
  const int stop = decided ? sc->stop : res <= sc->tol ? 1 : it >= sc->max_iter ? 2 : 0;
  const bool conv = stop == 1, fail = stop == 2, no_z = decided && stop;
  const double gz = no_z ? 0.0 : red ? red[1] : gz_part ? sum_partials(gz_part, sh, gz_n) : sum_partials(partials_in + kMaxPartials, sh);
  // (decided == 2: the other workgroups may still be reading sc->gg while workgroup 0 stores it here - the very value it has just read, so the race is harmless)
  if (blockIdx.x == 0 && threadIdx.x == 0) { sc->gg = gg; if (!no_z) sc->gz = gz; sc->res = res; sc->it = it; }
  if (conv || fail) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_u; i += (int64_t)gridDim.x * kBlock) x[i] = fma(alpha, d[i], x[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc->converged = conv ? 1 : 0; sc->finishing = 1; }
    return;
  }
  const double beta = gz / gh_old;
  PORO_OCT_LOOP(D) {          // (two positions per thread, as in k_fdmo_update_g2, were measured here too: 72 instead of 59 us, and 111 instead of 70 us with d resident and x streamed - the paired read-modify-writes of the nodal vectors cost more than the 16-byte octant reads save)
    PORO_OCT_DECODE(D)
    double w[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) w[o] = part_on<PD>(D, o) ? z[(int64_t)(c * D.no + part_at<PD>(D, o)) * D.co + idx] : 0.0;
    bfly_bwd(w, P.centre);
#pragma unroll
    for (int m = 0; m < 8; ++m) if (P.live[m]) {
      const int64_t dof = P.node[m] * NC + c;
      const double dv = d[dof], xv = XNT ? __builtin_nontemporal_load(&x[dof]) : x[dof];
      if (XNT) __builtin_nontemporal_store(fma(alpha, dv, xv), &x[dof]); else x[dof] = fma(alpha, dv, xv);
      d[dof] = fma(beta, dv, -w[m]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { sc->beta = beta; sc->gh2[parity ^ 1] = gz; }
}

// block partials of a . b over the planes this rank owns (slab form: the upper shared plane is the neighbour's)
__global__ void __launch_bounds__(kBlock) k_fdmo_dot_owned(OctDims D, const double *__restrict__ a, const double *__restrict__ b, double *partials, const PcgScalars *gate) {
  __shared__ double sh[5];
  if (gate && (gate->done | gate->finishing)) return;
  // every block of a, b is [plane][position]: the owned planes are its leading part (row pads are zeros in both)
  const int64_t per = (int64_t)D.own_z * D.hxp * D.hy;          // (hxp even: pairs)
  const int nblk = D.nc * D.no, share = gridDim.x / nblk, blk = blockIdx.x / max(share, 1), sub = blockIdx.x - blk * share;   // workgroups per block of the arrays; the remainder idles
  double acc = 0;
  if (share > 0 && blk < nblk) {
    const double2 *__restrict__ a2 = reinterpret_cast<const double2 *>(a + blk * D.co), *__restrict__ b2 = reinterpret_cast<const double2 *>(b + blk * D.co);
    for (int64_t e = (int64_t)sub * kBlock + threadIdx.x; e < per / 2; e += (int64_t)share * kBlock) { const double2 u = a2[e], v = b2[e]; acc = fma(u.x, v.x, fma(u.y, v.y, acc)); }
  }
  acc = block_sum(acc, sh);
  store_partial(partials, acc);
}

// ---- slab form: the z transform needs whole global lines.  Columns = (component, quadrant, plane position), grouped in chunks of cw; rank q transforms chunks
//      [q cps, (q + 1) cps).  Two all-to-alls of [rank][plane][share column] buffers; the z butterfly rides in the unpack / pack next to the transposed array ----
struct SlabGeo { int cw, nchunk, cps, chunk_total, rank, my_chunks, hzg, ng, np; int64_t scols, pl, co; };
// transposed array -> send buffer: every rank's planes (shared ones to both owners), v_k = a + b, v_k' = a - b
__global__ void __launch_bounds__(256) k_fdmo_slab_scatter_pack(SlabGeo S, int rows, const int64_t *__restrict__ row_out, const int32_t *__restrict__ row_kz,
                                                                  const double *__restrict__ tz, double *__restrict__ buf, const PcgScalars *gate) {
  if (gate && (gate->done | gate->finishing)) return;
  const int per_row = S.my_chunks * S.cw, total = rows * per_row;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int row = e / per_row, col = e - row * per_row, cl = col / S.cw, j = col - cl * S.cw;
    const int kz = row_kz[row];
    if (S.np == 1) { buf[row_out[row] + col] = tz[((int64_t)cl * S.hzg + kz) * S.cw + j]; continue; }     // (scalar systems: no parity split)
    const int mz = S.ng - 1 - kz, kh = min(kz, mz);
    const double a = tz[((int64_t)(2 * cl) * S.hzg + kh) * S.cw + j], b = tz[((int64_t)(2 * cl + 1) * S.hzg + kh) * S.cw + j];
    buf[row_out[row] + col] = kz == mz ? a : (kz < mz ? a + b : a - b);
  }
}

// ---- the transform pass --------------------------------------------------------------------------------------------------------------------
struct OctPass {
  int mode;                 // 0: contract columns, then rows (pass 1); 1: rows, eigenvalue scaling, rows (pass 2); 2: rows, then columns (pass 3)
  int R, C;                 // valid rows / columns of a block (mode 1: C = columns of a full chunk, the last chunk has fewer)
  int kk1, kk2;             // k-steps (of 4) of the two GEMMs
  int nblk;                 // blocks per (component, octant)
  int64_t co_stride, blk_stride, row_stride;
  int bit1, bit2;           // octant bit that selects the parity of the matrices of GEMM 1 / 2
  int pl;                   // mode 1: columns of a plane = row pitch x hy
  const void *T1[3][2], *T2[3][2];                       // [component][parity], MFMA fragment order [tile][4 NT][64]: doubles (k_fdmo_pass, k_fdmo_zpass_both) or floats (k_fdmo_pass_f32)
  const double *lam_z[3][2]; double cz[3]; const double *bxy;   // mode 1: eigenvalues of the line direction; bxy[(4 c + (o & 3)) pl + column] = the other two directions' share
  const double *in_blk[3]; double *out_blk[3]; int use_in_off, use_out_off;   // batched scalar systems (no_shift = 0, up to 3 blocks = right-hand sides in separate vectors): every block's own vector instead of `in` / `out` + block * co_stride
  int bxy_cmul;                 // bxy table: blocks per component (4: displacement system; 0: the scalar systems share one table)
  int no_shift;                 // log2 of the blocks per component (3: octants, 2: quadrants of the slab form, 0: scalar system)
  int slab_z /* parity parts of the transposed blocks: 2, or 1 for the scalar systems; 0: not the slab form */, chunk0, chunk_total, nchunk;   // slab form, pass 2: workgroup = (local chunk, z parity) of the transposed array; its global chunk number gives (component, quadrant, chunk of the plane)
  // slab form: the copies around the all-to-alls ride in the passes.  The exchange buffer is [send | recv], each [rank q][plane][share column]; column X = (block) nchunk cw +
  // plane position belongs to rank q = X / scols, so its address is X + q (pitch - 1) scols + plane scols: pass 1 (slab_io = 1) stores there (planes >= store_planes are the
  // neighbour's and are not sent; the own share goes straight to the receive half), pass 3 (slab_io = 2) loads the scattered planes from there; pass 2 (row_in): offset of every
  // global plane in the gathered buffer - the block is loaded as even / odd combination of a plane and its mirror image
  int slab_io, store_planes, ng, scols, col_unit, rank; float inv_scols; int64_t dest_stride, recv_off; const int64_t *row_in;
  int vec2;                     // rows are 16-byte aligned (even pitch, even chunk offsets): 16-byte block loads; 0: 8-byte loads (the scalar Q1 systems keep their nodal layout)
  int per_dir, bitz;            // per-direction form (VAR = 3): the descriptor is one of its passes; bit of a part's index that selects the parity of lam_z (a whole z line: both slots hold the one table)
  double *gz_part;              // octant form, pass 2 (GZ instantiations): one partial sum of g . z per workgroup, see the epilogue of the first GEMM
  const PcgScalars *gate;       // inside a PCG iteration: the launch is a no-op once the solve has finished (the host enqueues iterations ahead of the device-side stopping test)
  PcgStopTest stop;             // pass 1 as the first kernel of a preconditioner call inside PCG: the iteration's stopping test (common.hpp); gg_part == null elsewhere
  unsigned long long *stamps;   // diagnostic (PORO_FDMO_STAMPS): per block 8 words: 100 MHz time at start / block in LDS / GEMM 1 done / intermediate in LDS / GEMM 2 done / stored, HW_ID, XCC_ID
};

// (kFdmoMaxTiles, fdm_tables.hpp: 16-wide tiles per line the transform kernel is instantiated for - half lines, or whole lines of the per-direction form, of <= 128 entries)
template <int NT> constexpr int pass_waves() { return NT == 5 ? 4 : NT; }   // waves of a workgroup: one per tile row / column, except NT = 5 (four waves share 25 tiles)
template <int NT> struct PassGeom {
  static constexpr int PADN = 16 * NT, KKP = 4 * NT;
  static constexpr int LDA = PADN + 2;                       // data as the A operand: lane (i, kq) reads [16 t + i][4 kk + kq]; LD = 2 * odd (mod 32) keeps a 32-lane group on 32 bank pairs
  static constexpr int LDB = PADN + ((NT & 1) ? 0 : 16);     // data as the B operand: lane (j, kq) reads [4 kk + kq][16 w + j]; LD = 16 (mod 32)
  static constexpr int LDMAX = LDA > LDB ? LDA : LDB;
  // Both leading dimensions count ELEMENTS and serve the 8-byte elements of k_fdmo_pass and the 4-byte ones of k_fdmo_pass_f32 alike.  A fragment read is serviced in two
  // groups of 32 lanes (kq = 0, 1 and kq = 2, 3).  Doubles (ds_read_b64): bank = (byte address / 4) mod 64 - an element is a bank PAIR, 32 pairs.  Floats (ds_read_b32):
  // bank = (byte address / 4) mod 32 - an element is a bank, 32 banks.  Either way a group is conflict-free iff its 32 element offsets differ mod 32.
  //   A role: offsets i LD + kq (i < 16, kq in {0, 1}); LD = 2 * odd (mod 32) -> (2 i * odd + kq) mod 32 takes every value once.
  //   B role: offsets kq LD + j (j < 16); LD = 16 (mod 32) -> j and j + 16.
  // fp32 accumulator stores (one register of all lanes: rows 4 kq + q, element offsets j + 4 kq LD): 4 LD = 0 or 8 (mod 32), two lanes per bank in a group of 32 - the 2-way
  // conflict that ds_write_b32 absorbs in its own issue cycles.  LD is even: the float2 stores of the staged block are 8-byte aligned.
};

// One item (= one (component, octant, block)) per workgroup; the hardware dispatcher balances the items over the CUs.
// Workgroup shape (census of resident workgroups per CU, profiles/r03_lds_residency.txt): a 5-wave workgroup - the natural shape for 5 x 5 tiles - is given the
// registers of an 8-wave one (two slots on every SIMD), which left 1.2-2 workgroups resident and the matrix pipe idle 55 % of the time (profiles/r03_fdmo_stamps_v1.txt).
// 4-wave workgroups keep three resident at up to 128 registers, one wave of each on every SIMD.  So for NT = 5 FOUR waves share the tiles:
//   passes 1 / 3 (5 x 5 tiles): wave w owns tile row (or column) w in full plus tile (4, w) [(w, 4)]; tile (4, 4) goes to the wave whose number equals the item number
//     mod 4, so that over the items every SIMD gets the same share (6.25 tiles per wave on average; the two GEMM bodies - with and without the seventh tile - are
//     separate branch-free instruction streams);
//   pass 2 (lines are independent): chunks of 64 columns = 5 x 4 tiles, wave w owns (w, 0..3) and (4, w): five tiles each, nothing left over.
// VAR is stated by the host code that builds the descriptor (PassVariant; launch_pass_nt rejects a descriptor whose flags contradict it):
// VAR = 0: the octant form on one rank (24 blocks, aligned rows, no exchange buffer, no per-block offsets) with those switches folded at compile time;
// VAR = 1: the quadrant form of the displacement system on slabs (pass 1 stores into / pass 3 loads from the exchange buffer, pass 2 forms the parity parts on load), likewise;
// VAR = 2: everything else by run-time switches (scalar systems, batched right-hand sides)
// VAR = 3: the per-direction form of the displacement system on one rank (PORO_FDM_FORM_PER_DIRECTION): VAR = 0 with 2^(split directions) parts per component instead of
//          eight.  The same folded switches; what differs is data: the part count (no_shift), the planes of the bxy table per component (bxy_cmul = 2^(split among x, y)), and
//          which bit of the part's index selects the parity of each matrix set (bit1 / bit2 / bitz).  A whole direction has one matrix set, which the descriptor lists in both
//          parity slots, so the kernel selects as always.  It keeps GZ, the pass-1 stopping test (QUARTERS included) and the in-place operation of VAR = 0
// GZ (MODE = 1, VAR = 0 and 3 only): the pass also leaves g . z.  Per block z = B Lambda^-1 F g with B = F^T (fdmo_upload_dir), so sum Q_g Q_z = sum over the modes of
// ghat^2 / den with ghat = (F x F x F) Q_g - which is what the accumulators hold after the first GEMM, next to the 1 / den that scales them.  Removed modes give
// 1 / den = 0, pads are exact zeros and every tile of pass 2 belongs to one wave, so the workgroup's sum is its share of g . z: two FMAs per entry and one
// 8-byte store, no extra load, no extra launch (P.gz_part[blockIdx.x]; k_fdmo_update_d adds the slots up in a fixed order)
// In place (in == out; `in` and `out` carry no __restrict__): every workgroup loads exactly the R x C entries of its block that it stores, blocks of different workgroups are
// disjoint, and the block is staged in full before the first store - all global loads of the input sit in the staging loop, whose values are in LDS by the barrier in front
// of the first GEMM, and nothing but LDS and the transform matrices is read after it.  So pass 2 AND passes 1 / 3 may overwrite their input; the single-rank octant form in
// fp64 runs g -> z, z -> z, z -> z without a scratch array (fdmo_apply).  Pad column: passes 1 and 3 of the displacement forms store it too (C = the row pitch, plan_pass) -
// exact zeros, because the pad rows of the transform matrices are zero (pack_fragments) and the staged data are finite.  Pass 1 therefore rewrites every entry of the
// array it stores into, pads included, whatever that array held before (the octant form's z doubles as the operator's output h, ctx.hip: solve_u_fdm).
template <int NT, int MODE, int VAR, bool GZ = false>
__global__ void __launch_bounds__(64 * pass_waves<NT>())
k_fdmo_pass(OctPass P, const double *in, double *out) {
  static_assert(!GZ || (MODE == 1 && (VAR == 0 || VAR == 3)), "g . z comes out of pass 2 of the single-rank octant and per-direction forms only");
  // (the kernel argument stays in the kernarg segment - a modified copy would live in scratch because of its dynamically indexed members)
  constexpr bool GENERAL = VAR == 2, SLAB = VAR == 1, PERDIR = VAR == 3;
  const int f_vec2 = GENERAL ? P.vec2 : 1, f_slab_z = GENERAL ? P.slab_z : (SLAB && MODE == 1 ? 2 : 0), f_slab_io = GENERAL ? P.slab_io : (SLAB && MODE == 0 ? 1 : SLAB && MODE == 2 ? 2 : 0),
            f_use_in = GENERAL ? P.use_in_off : 0, f_use_out = GENERAL ? P.use_out_off : 0, f_no_shift = (GENERAL || PERDIR) ? P.no_shift : (SLAB ? 2 : 3), f_bxy_cmul = (GENERAL || PERDIR) ? P.bxy_cmul : 4;
  const int64_t *const f_row_in = (GENERAL || (SLAB && MODE == 1)) ? P.row_in : nullptr;
  typedef PassGeom<NT> Gm;
  constexpr int NW = pass_waves<NT>();                       // waves
  constexpr bool EXTRA = NT > NW;                            // NT == 5: the fifth tile row / column is shared out
  constexpr int XT = NT - 1;                                 // index of that tile row / column
  constexpr int NL = (MODE == 1 && EXTRA) ? NW : NT;         // tiles a wave loops over beside its own (pass 2: column tiles of a chunk)
  constexpr bool CORNER = EXTRA && MODE != 1;                // tile (XT, XT) exists
  constexpr int NACC = NL + (EXTRA ? 1 : 0) + (CORNER ? 1 : 0);
  constexpr bool kColsFirst = MODE == 0, kColsSecond = MODE == 2;
  constexpr int LD1 = kColsFirst ? Gm::LDA : Gm::LDB, LD2 = kColsSecond ? Gm::LDA : Gm::LDB;
  constexpr int NS = EXTRA ? 2 : 1;                          // fragment streams per wave: its own tile row of T (and the shared one)
  constexpr int PADC = 16 * NL;                              // padded block columns
  extern __shared__ double L[];                              // PADN x LDMAX doubles (dynamic: more than 64 KB from NT = 6 on)
  __shared__ double gz_wave[GZ ? NW : 1];                    // (referenced by the GZ instantiations only: the others allocate nothing for it)
  // pass 1 as the first kernel of a preconditioner call inside PCG: the iteration's stopping test (PcgStopTest).  It replaces the read of `stop`, which workgroup 0 of this
  // very launch writes.  Its inputs are requested in front of the gate's own loads, so that the two latencies overlap, and the decision falls before the block is staged:
  // the test's registers are free again by then (held across the staging loads they cost the five-tile pass its third resident workgroup)
  // Four-wave workgroups (QUARTERS) share the sum out instead: each wave adds a quarter of the partials (8 registers, requested with the staging loads), the four wave sums
  // meet in LDS at the staging barrier and the decision falls behind it - a workgroup that stops has stored nothing by then.  P.stop.per_wave keeps the form above (A/B hook)
  // (the Octant and PerDirection variants only: the slab form refuses a stopping test and the scalar passes are handed none, so their pass 1 keeps the form above and pays nothing for this one)
  constexpr bool QUARTERS = MODE == 0 && (VAR == 0 || VAR == 3) && NW == 4;
  __shared__ double stop_wave[QUARTERS ? 4 : 1];             // (referenced by the QUARTERS instantiations only)
  [[maybe_unused]] PcgStopQuarter stop_q; [[maybe_unused]] bool stop_pending = false;
  if (MODE == 0 && P.stop.gg_part) {
    if (QUARTERS && !P.stop.per_wave) {
      if (P.gate && (P.gate->done | P.gate->finishing)) return;
      pcg_stop_load_quarter(P.stop, stop_q); stop_pending = true;
    } else {
      PcgStopInputs stop_in;
      pcg_stop_load(P.stop, stop_in);
      if (P.gate && (P.gate->done | P.gate->finishing)) return;
      if (pcg_stop_decide(P.stop, stop_in)) return;
    }
  } else if (pcg_gate_closed(P.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  int b, c, o, co = 0; int64_t base;
  if (MODE == 1 && f_slab_z) {
    const int G = P.chunk0 + (int)(blockIdx.x >> (f_slab_z - 1)), cq = G / P.nchunk;
    if (G >= P.chunk_total) return;                                  // (the last rank's share may be short; workgroup-uniform, before any barrier)
    b = G - cq * P.nchunk; c = cq >> 2; o = (cq & 3) | ((blockIdx.x & (f_slab_z - 1)) << 2); base = (int64_t)blockIdx.x * P.blk_stride;
  } else {
    co = blockIdx.x / P.nblk;
    b = blockIdx.x % P.nblk; c = co >> f_no_shift; o = co & ((1 << f_no_shift) - 1); base = (int64_t)co * P.co_stride + (int64_t)b * P.blk_stride;
  }
  const int64_t base_in = f_use_in ? (int64_t)b * P.blk_stride : base, base_out = f_use_out ? (int64_t)b * P.blk_stride : base;
  if (f_use_in) in = P.in_blk[co];
  if (f_use_out) out = P.out_blk[co];
  const bool heavy = CORNER && w == (int)(blockIdx.x & (NW - 1));   // this wave also computes tile (XT, XT)
  const int R = P.R, C = MODE == 1 ? min(P.C, P.pl - b * P.C) : P.C;
  const double *__restrict__ T1 = static_cast<const double *>(P.T1[c][(o >> P.bit1) & 1]) + lane, *__restrict__ T2 = static_cast<const double *>(P.T2[c][(o >> P.bit2) & 1]) + lane;
  // slab form: address of plane position `col` of this block in the exchange buffer
  // (a block's columns lie in at most two shares when a share is at least a block long - up to 12 ranks: the two bases are wave-uniform scalars)
  int slab_q0 = 0, slab_sw = 0; int64_t slab_base[2] = {0, 0};
  if (MODE != 1 && f_slab_io) {
    const int X0 = co * P.col_unit; slab_q0 = X0 / P.scols; slab_sw = (slab_q0 + 1) * P.scols - X0;
    for (int k = 0; k < 2; ++k) slab_base[k] = (int64_t)X0 + (int64_t)(slab_q0 + k) * P.dest_stride + (int64_t)b * P.scols + ((f_slab_io == 2 || slab_q0 + k == P.rank) ? P.recv_off : 0);
  }
  auto slab_at = [&](int col) -> int64_t {
    if (P.scols >= P.col_unit) return (int64_t)col + (col >= slab_sw ? slab_base[1] : slab_base[0]);
    const int X = co * P.col_unit + col;
    int q = (int)((float)X * P.inv_scols); q -= q * P.scols > X; q += (q + 1) * P.scols <= X;      // X / scols (X < 2^24)
    return (int64_t)X + (int64_t)q * P.dest_stride + (int64_t)b * P.scols + ((f_slab_io == 2 || q == P.rank) ? P.recv_off : 0);
  };
  auto stamp = [&](int k) { if (P.stamps && tid == 0) P.stamps[(int64_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime(); };
  stamp(0);
  // ---- block -> LDS, zero padded to PADN x PADC (the padding meets zero columns of T, but must be finite).  Rows are 16-byte aligned (even pitch, even chunk
  //      offsets, even C): 16-byte loads and LDS stores, all loads in flight before the first LDS store ----
  {
    constexpr int HP = PADC / 2, TOT = Gm::PADN * HP, PER = (TOT + 64 * NW - 1) / (64 * NW);
    double2 stage[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP);
      if (MODE == 1 && f_row_in) {             // gathered planes -> parity part of the global line: e_k = v_k + v_k', o_k = v_k - v_k' (centre plane: e = v, o = 0)
        const bool ok = e < TOT && r < R && c2 < C, split = f_slab_z == 2; const int rr = ok ? r : 0, mr = split ? P.ng - 1 - rr : rr; const int64_t cb = (int64_t)(blockIdx.x >> (f_slab_z - 1)) * P.C + c2;
        const double2 lo = ok ? *reinterpret_cast<const double2 *>(in + f_row_in[rr] + cb) : double2{0.0, 0.0}, hi = (ok && mr != rr) ? *reinterpret_cast<const double2 *>(in + f_row_in[mr] + cb) : double2{0.0, 0.0};
        const bool odd = split && (blockIdx.x & 1);
        stage[u].x = odd ? (mr != rr ? lo.x - hi.x : 0.0) : lo.x + hi.x; stage[u].y = odd ? (mr != rr ? lo.y - hi.y : 0.0) : lo.y + hi.y;
      } else if (MODE == 2 && f_slab_io == 2) {
        if (f_vec2) stage[u] = (e < TOT && r < R && c2 < C) ? *reinterpret_cast<const double2 *>(in + slab_at(r * (int)P.row_stride + c2)) : double2{0.0, 0.0};
        else { stage[u].x = (e < TOT && r < R && c2 < C) ? in[slab_at(r * (int)P.row_stride + c2)] : 0.0; stage[u].y = (e < TOT && r < R && c2 + 1 < C) ? in[slab_at(r * (int)P.row_stride + c2 + 1)] : 0.0; }
      }
      else if (f_vec2) stage[u] = (e < TOT && r < R && c2 < C) ? *reinterpret_cast<const double2 *>(in + base_in + (int64_t)r * P.row_stride + c2) : double2{0.0, 0.0};
      else { const double *src = in + base_in + (int64_t)r * P.row_stride + c2; stage[u].x = (e < TOT && r < R && c2 < C) ? src[0] : 0.0; stage[u].y = (e < TOT && r < R && c2 + 1 < C) ? src[1] : 0.0; }
    }
    if constexpr (QUARTERS) { if (stop_pending) pcg_stop_post_quarter(stop_q, stop_wave); }   // (the partials were requested first: they are here before the block is)
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP); if (e < TOT) *reinterpret_cast<double2 *>(&L[r * LD1 + c2]) = stage[u]; }
  }
  // transform-matrix fragments in two rotating register buffers of 4 k-steps: the 2 NT chunks of the two GEMMs form one sequence, and a buffer is refilled with the
  // chunk after next as soon as the MFMAs that used it have been issued
  // (deeper buffers for the General variant, whose launches never fill the chip - half a GEMM or a whole one per buffer - were measured and are SLOWER there: DESIGN, "Latency-bound work")
  constexpr int CHK = EXTRA ? 2 : 4, NCH = Gm::KKP / CHK;     // k-steps per chunk (two fragment streams at NT = 5: smaller chunks keep the kernel within the registers of three resident workgroups), chunks per GEMM
  double tf[2][NS][CHK];
  auto load_chunk = [&](int buf, int step) {                 // step < NCH: chunk `step` of T1, else chunk step - NCH of T2
    const double *__restrict__ T = step < NCH ? T1 : T2; const int ch = step < NCH ? step : step - NCH;
#pragma unroll
    for (int k = 0; k < CHK; ++k) {
      tf[buf][0][k] = T[((int64_t)w * Gm::KKP + CHK * ch + k) * 64];
      if constexpr (EXTRA) tf[buf][1][k] = T[((int64_t)XT * Gm::KKP + CHK * ch + k) * 64];
    }
  };
  v4d acc[NACC];
  auto zero_acc = [&]() {
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = v4d{0, 0, 0, 0};
  };
  // one GEMM = NCH chunks of CHK k-steps.  Every tile of the padded problem is computed (the padding is exact zeros: no predicates inside), only whole trailing k-steps are skipped.
  //   contract columns: acc[t] = tile (t, w) = sum_k data(rows of tile t, k) T(rows of tile w, k); extra: acc[NL] = tile (w, XT), acc[NL + 1] = tile (XT, XT)
  //   contract rows:    acc[u] = tile (w, u) = sum_k T(rows of tile w, k) data(k, columns of tile u); extra: acc[NL] = tile (XT, w), acc[NL + 1] = tile (XT, XT)
  auto gemm = [&](auto contract_cols, auto ld_c, auto first_step_c, auto corner_c, int kk_n) {
    constexpr bool kCols = decltype(contract_cols)::value, kCorner = decltype(corner_c)::value; constexpr int LD = decltype(ld_c)::value, S0 = decltype(first_step_c)::value;
    const double *La = kCols ? L + j * LD + kq : L + kq * LD + j;
    const double *Lw = kCols ? La + 16 * w * LD : La + 16 * w;                 // this wave's own tile row / column of the data (runtime w)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int buf = (S0 + ch) & 1;
#pragma unroll
      for (int k = 0; k < CHK; ++k) {
        const int kk = CHK * ch + k;
        if (kk < Gm::KKP - 3 || kk < kk_n) {                 // (kk_n >= KKP - 3 always: wave-uniform branches on the last three k-steps only)
          double d[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) if (t < NL || (kCorner && t == XT)) d[t] = kCols ? La[16 * t * LD + 4 * kk] : La[4 * kk * LD + 16 * t];
          double dw = 0; if constexpr (EXTRA) dw = kCols ? Lw[4 * kk] : Lw[4 * kk * LD];
#pragma unroll
          for (int t = 0; t < NL; ++t) acc[t] = kCols ? __builtin_amdgcn_mfma_f64_16x16x4f64(d[t], tf[buf][0][k], acc[t], 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(tf[buf][0][k], d[t], acc[t], 0, 0, 0);
          if constexpr (EXTRA) acc[NL] = kCols ? __builtin_amdgcn_mfma_f64_16x16x4f64(dw, tf[buf][1][k], acc[NL], 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(tf[buf][1][k], dw, acc[NL], 0, 0, 0);
          if constexpr (kCorner) acc[NL + 1] = kCols ? __builtin_amdgcn_mfma_f64_16x16x4f64(d[XT], tf[buf][1][k], acc[NL + 1], 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(tf[buf][1][k], d[XT], acc[NL + 1], 0, 0, 0);
        }
      }
      if (S0 + ch + 2 < 2 * NCH) load_chunk(buf, S0 + ch + 2);
    }
  };
  // accumulator a holds tile (tr, tc): element (16 tr + 4 q + kq, 16 tc + j)
  auto tile_of = [&](int a, int &tr, int &tc, bool cols) {
    if (a < NL) { tr = cols ? a : w; tc = cols ? w : a; }
    else if (a == NL) { tr = cols ? w : XT; tc = cols ? XT : w; }
    else { tr = XT; tc = XT; }
  };
  typedef std::integral_constant<bool, kColsFirst> CF; typedef std::integral_constant<int, LD1> L1c;
  typedef std::integral_constant<bool, kColsSecond> CS; typedef std::integral_constant<int, LD2> L2c;
  typedef std::integral_constant<int, 0> S0c; typedef std::integral_constant<int, NCH> S1c;
  __builtin_amdgcn_s_setprio(3);   // the few instructions of the load phase go ahead of the co-resident workgroups' matrix streams
  load_chunk(0, 0); load_chunk(1, 1);
  zero_acc();
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();
  if constexpr (QUARTERS) { if (stop_pending && pcg_stop_decide_quarters(P.stop, stop_q, stop_wave)) return; }   // (workgroup-uniform; the block and fragment loads are out, but nothing is stored outside LDS yet - bar the diagnostic stamp(0))
  stamp(1);
  if (heavy) gemm(CF{}, L1c{}, S0c{}, std::integral_constant<bool, CORNER>{}, P.kk1); else gemm(CF{}, L1c{}, S0c{}, std::false_type{}, P.kk1);
  __syncthreads();                                   // everybody has finished reading the input block
  stamp(2);
  // ---- first result -> LDS in the layout of the second GEMM (MODE 1: divided by the eigenvalue sums on the way) ----
  if constexpr (MODE == 1) {
    // rows of this wave's tiles: tile row w (and the shared row XT); columns: tile column of the accumulator.  One entry at a time (sched_barrier), otherwise the
    // reciprocal sequences of all of them pile up in registers
    const double *lamz = P.lam_z[c][(o >> (PERDIR ? P.bitz : 2)) & 1], *bx = P.bxy + (int64_t)(f_bxy_cmul * c + (PERDIR ? (o & (P.bxy_cmul - 1)) : (o & 3))) * P.pl;   // (per-direction form: the x / y bits are the lowest of a part's index)
    const double czc = P.cz[c];
    double lzw[4], lzx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { lzw[q] = czc * lamz[16 * w + 4 * q + kq]; lzx[q] = EXTRA ? czc * lamz[16 * XT + 4 * q + kq] : 0.0; }
    double gz = 0;                      // GZ: this thread's share of g . z
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int tr, tc; tile_of(a, tr, tc, false);
      const double bxy = bx[min(b * P.C + 16 * tc + j, P.pl - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // reciprocal by v_rcp_f64 + one Newton step; modes that do not exist carry lam = inf and give exactly 0
        const double den = (a < NL ? lzw[q] : lzx[q]) + bxy;
        double r = __builtin_amdgcn_rcp(den);
        r = den < 1e300 ? fma(r, fma(-den, r, 1.0), r) : 0.0;
        const double zh = acc[a][q] * r;
        L[(16 * tr + 4 * q + kq) * LD2 + 16 * tc + j] = zh;
        if constexpr (GZ) gz = fma(acc[a][q], zh, gz);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (GZ) {                 // wave sums -> LDS; the barrier in front of the second GEMM publishes them
      gz = wave_sum(gz);
      if (lane == 0) gz_wave[w] = gz;
    }
  } else {
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int tr, tc; tile_of(a, tr, tc, kColsFirst);
      if (a == NL + 1 && !heavy) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) L[(16 * tr + 4 * q + kq) * LD2 + 16 * tc + j] = acc[a][q];
    }
  }
  zero_acc();
  __syncthreads();
  stamp(3);
  if constexpr (GZ) {
    if (tid == 0) { double t = 0; for (int k = 0; k < NW; ++k) t += gz_wave[k]; P.gz_part[blockIdx.x] = t; }   // fixed order: bitwise reproducible
  }
  if (heavy) gemm(CS{}, L2c{}, S1c{}, std::integral_constant<bool, CORNER>{}, P.kk2); else gemm(CS{}, L2c{}, S1c{}, std::false_type{}, P.kk2);
  if (P.stamps) { __syncthreads(); stamp(4); }
  // ---- store ----
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    int tr, tc; tile_of(a, tr, tc, kColsSecond);
    if (a == NL + 1 && !heavy) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * tr + 4 * q + kq, cc = 16 * tc + j;
      if (MODE == 0 && f_slab_io == 1) { if (r < R && cc < C && b < P.store_planes) out[slab_at(r * (int)P.row_stride + cc)] = acc[a][q]; }
      else if (r < R && cc < C) out[base_out + (int64_t)r * P.row_stride + cc] = acc[a][q];
    }
  }
  if (P.stamps) {
    __builtin_amdgcn_s_waitcnt(0); __syncthreads(); stamp(5);
    if (tid == 0) { unsigned hw, xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc)); P.stamps[(int64_t)blockIdx.x * 8 + 6] = hw; P.stamps[(int64_t)blockIdx.x * 8 + 7] = xcc; }
  }
}

// ---- the class-split passes of the octant form (one rank, fp64; uniform Q2 lines with equal ends: class_split_tables, fdm_tables.hpp) --------------------------------
// Every half-line transform F = S W: two class transforms (vertex / midpoint positions, half the length each) and a 2 x 2 mix per frequency.  The three passes become
//   pass 1: read g (nodal half-line order), x forward, mix, y forward, mix      -> class-major modes in x and y
//   pass 2: z forward, mix, scale, transposed mix, z backward                   (in place; z stays nodal at the interfaces)
//   pass 3: transposed mixes, y backward, x backward                            -> z in nodal half-line order
// so g and z keep their layout for the CG vector kernels; the order between the passes is private: slot s of the vertex class at index s, of the midpoint class at
// nv + s - compact, the same hy x hxp planes.  In LDS a line of 16 NT entries is two class regions of H = 8 NT: position / slot p of the vertex class at p, of the
// midpoint class at H + p (node 2 p / 2 p + 1 of the nodal order).  A class GEMM contracts over its own region only: (nv + 3) / 4 and (nm + 3) / 4 k-steps instead of 4 NT.
// A wave always holds tile t of BOTH classes (for some batch tiles): the two partners of a frequency sit in the same lane and accumulator slot of accv / accm, so every
// forward mix is two FMAs per entry in registers.  The transposed mixes of pass 3 act on its input: they ride in its staging loop.
// Kept from k_fdmo_pass<.., 0>: in-place operation (the block is staged in full before the first store, blocks are disjoint), the gate, the stopping test of pass 1
// (pcg_stop_load / pcg_stop_decide: the bits of every other form of the test), g . z out of pass 2 as the sum of ghat^2 / den in a fixed order with one slot per workgroup
// of the same grid, exact zeros from removed modes (1 / den = 0, zero mix) and pads (zero rows of the class transforms), no scratch.
struct OctPassVM {
  int mode, R, C, nblk, pl;           // as in OctPass
  int64_t co_stride, blk_stride, row_stride;
  int bit1, bit2;                     // octant bit that selects the parity of the tables of GEMM 1 / 2
  int kkv[2], kkm[2];                 // k-steps of the vertex / midpoint class in GEMM 1 / 2
  int nvx, nvy, nmy;                  // passes 1 / 3: vertex positions of an x line (= index of the first midpoint slot in the compact order), vertex / midpoint positions of a y line
  const double *Tv[2][3][2], *Tm[2][3][2];     // [GEMM][component][parity]: class transforms in fragment order [(NT + 1) / 2 tiles][2 NT k-steps][64]
  const double *mix[2][3][2];         // [GEMM][component][parity]: [slot][4] of the direction of that GEMM
  const double *lam_z[3][2];          // pass 2: [class][64] eigenvalues by slot
  double cz[3]; const double *bxy;    // bxy in the compact class-major order of the plane
  double *gz_part; const PcgScalars *gate; PcgStopTest stop;
};
template <int NT> constexpr int vm_waves() { return NT == 5 ? 4 : (NT + 1) / 2; }      // one per class-tile pair; NT = 5: four, one per SIMD (see the roles in the kernel)
// registers: three workgroups per CU fit the LDS up to NT = 5 (PassGeom), so their waves must fit three to a SIMD - 168 registers; beyond, the accumulators alone need more
template <int NT> constexpr int vm_waves_per_simd() { return NT <= 5 ? 3 : NT == 6 ? 2 : 1; }
template <int NT, int MODE, bool GZ = false>
__global__ void __launch_bounds__(64 * vm_waves<NT>()) __attribute__((amdgpu_waves_per_eu(vm_waves_per_simd<NT>())))
k_fdmo_pass_vm(OctPassVM P, const double *in, double *out) {
  static_assert(!GZ || MODE == 1, "g . z comes out of pass 2");
  typedef PassGeom<NT> Gm;
  constexpr bool QUAD = NT == 5;
  constexpr int NW = vm_waves<NT>(), NCT = (NT + 1) / 2, H = 8 * NT, KK = 2 * NT, PADN = Gm::PADN;
  constexpr int NB = MODE == 1 ? (NT == 5 ? 4 : NT) : NT;      // batch tiles (pass 2: the columns of a chunk, pass2_chunk)
  constexpr bool kColsFirst = MODE == 0, kColsSecond = MODE == 2;
  constexpr int LD1 = kColsFirst ? Gm::LDA : Gm::LDB, LD2 = kColsSecond ? Gm::LDA : Gm::LDB;
  extern __shared__ double L[];                              // PADN x LDMAX doubles
  __shared__ double gz_wave[GZ ? NW : 1];
  if (MODE == 0 && P.stop.gg_part) {
    PcgStopInputs stop_in;
    pcg_stop_load(P.stop, stop_in);
    if (P.gate && (P.gate->done | P.gate->finishing)) return;
    if (pcg_stop_decide(P.stop, stop_in)) return;
  } else if (pcg_gate_closed(P.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int co = blockIdx.x / P.nblk, b = blockIdx.x % P.nblk, c = co >> 3, o = co & 7;
  const int64_t base = (int64_t)co * P.co_stride + (int64_t)b * P.blk_stride;
  const int R = P.R, C = MODE == 1 ? min(P.C, P.pl - b * P.C) : P.C;
  const int p1 = (o >> P.bit1) & 1, p2 = (o >> P.bit2) & 1;
  auto node_of = [](int r) { return r < H ? 2 * r : 2 * (r - H) + 1; };      // LDS line index -> nodal index
  // ---- block -> LDS, every entry of the padded block written once (the pads meet zero columns of the class transforms, but must be finite) ----
  if constexpr (MODE == 0) {            // nodal rows and columns -> class regions: a 16-byte load is one (vertex, midpoint) pair of a row
    constexpr int TOT = PADN * H, PER = (TOT + 64 * NW - 1) / (64 * NW);
    double2 stage[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / H, cp = e - r * H, rn = node_of(r);
      stage[u] = (e < TOT && rn < R && 2 * cp < C) ? *reinterpret_cast<const double2 *>(in + base + (int64_t)rn * P.row_stride + 2 * cp) : double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NW, r = e / H, cp = e - r * H; if (e < TOT) { L[r * LD1 + cp] = stage[u].x; L[r * LD1 + H + cp] = stage[u].y; } }
  } else if constexpr (MODE == 1) {     // nodal rows -> class regions, the columns of the chunk as they are
    constexpr int HP = 8 * NB, TOT = PADN * HP, PER = (TOT + 64 * NW - 1) / (64 * NW);
    double2 stage[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP), rn = node_of(r);
      stage[u] = (e < TOT && rn < R && c2 < C) ? *reinterpret_cast<const double2 *>(in + base + (int64_t)rn * P.row_stride + c2) : double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP); if (e < TOT) *reinterpret_cast<double2 *>(&L[r * LD1 + c2]) = stage[u]; }
  } else {                              // compact class-major modes -> class regions, with the transposed mixes of y and x: a thread takes the four partners of (y slot, x slot)
    constexpr int TOT = H * H, PER = (TOT + 64 * NW - 1) / (64 * NW);
    const int nvx = P.nvx, nmx = C - P.nvx, nvy = P.nvy, nmy = P.nmy;     // (C = the row pitch: the pad entry counts as a midpoint slot - it holds a zero)
    const double *__restrict__ my = P.mix[0][c][p1], *__restrict__ mx = P.mix[1][c][p2];
    double stage[PER][4];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, sy = e / H, sx = e - sy * H;
      const bool ok = e < TOT, rv = ok && sy < nvy, rm = ok && sy < nmy, cv = sx < nvx, cm = sx < nmx;
      const double *src = in + base + sx;
      stage[u][0] = (rv && cv) ? src[(int64_t)sy * P.row_stride] : 0.0;
      stage[u][1] = (rv && cm) ? src[(int64_t)sy * P.row_stride + nvx] : 0.0;
      stage[u][2] = (rm && cv) ? src[(int64_t)(nvy + sy) * P.row_stride] : 0.0;
      stage[u][3] = (rm && cm) ? src[(int64_t)(nvy + sy) * P.row_stride + nvx] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, sy = e / H, sx = e - sy * H;
      if (e < TOT) {
        const double2 y0 = *reinterpret_cast<const double2 *>(my + 4 * sy), y1 = *reinterpret_cast<const double2 *>(my + 4 * sy + 2);     // w_vv, w_mv | w_vm, w_mm
        const double2 x0 = *reinterpret_cast<const double2 *>(mx + 4 * sx), x1 = *reinterpret_cast<const double2 *>(mx + 4 * sx + 2);
        // transposed mix of y: class value = w_.v mode(v) + w_.m mode(m), column by column
        const double av_v = fma(y0.x, stage[u][0], y1.x * stage[u][2]), am_v = fma(y0.y, stage[u][0], y1.y * stage[u][2]);       // x slot of the vertex class
        const double av_m = fma(y0.x, stage[u][1], y1.x * stage[u][3]), am_m = fma(y0.y, stage[u][1], y1.y * stage[u][3]);       // x slot of the midpoint class
        // then of x, row by row
        L[sy * LD1 + sx] = fma(x0.x, av_v, x1.x * av_m); L[sy * LD1 + H + sx] = fma(x0.y, av_v, x1.y * av_m);
        L[(H + sy) * LD1 + sx] = fma(x0.x, am_v, x1.x * am_m); L[(H + sy) * LD1 + H + sx] = fma(x0.y, am_v, x1.y * am_m);
      }
    }
  }
  // ---- who computes what.  The result of a GEMM is NCT class-tile pairs x NB batch tiles; a wave holds some of them, both classes of a pair side by side in accv / accm.
  //   role A: the wave owns class tile `fixed` over batch tiles 0 .. NA-1 (one fragment of each class transform per k-step, NA data fragments);
  //   role B: the wave owns batch tile `fixed` over all NCT class tiles (NCT fragments of each class transform per k-step, one data fragment).
  // NT != 5: NCT waves, all role A over all batch tiles.  NT = 5 (QUAD; 3 class tiles, 5 batch tiles - 4 in pass 2): FOUR waves, one per SIMD, as for the dense pass
  // (profiles/r03_lds_residency.txt): passes 1 / 3: waves 0-2 role A over batch tiles 0-3, wave 3 role B on batch tile 4 (4 + 4 + 4 + 3 pair tiles); pass 2: every
  // wave role B on batch tile w (3 pair tiles each)
  constexpr int NA = QUAD ? 4 : NB, NACC = (QUAD && MODE == 1) ? NCT : NA, NTF = QUAD ? NCT : 1;
  const bool roleB = QUAD && (MODE == 1 || w == NW - 1);
  const int fixed = roleB ? (MODE == 1 ? w : NB - 1) : w;
  auto tile_of = [&](int a, int &ct, int &bt) { ct = roleB ? a : fixed; bt = roleB ? fixed : a; return a < (roleB ? NCT : NA); };
  // class-transform fragments in two rotating register buffers of CHK k-steps, as in k_fdmo_pass: the 2 NCH chunks of the two GEMMs form one sequence, and
  // a buffer is refilled with the chunk after next as soon as the MFMAs that used it have been issued
  constexpr int CHK = 2, NCH = KK / CHK;
  const double *__restrict__ T1v = P.Tv[0][c][p1] + lane, *__restrict__ T1m = P.Tm[0][c][p1] + lane, *__restrict__ T2v = P.Tv[1][c][p2] + lane, *__restrict__ T2m = P.Tm[1][c][p2] + lane;
  double tf[2][2][CHK][NTF];
  auto load_chunk = [&](auto role_c, int buf, int step) {    // step < NCH: chunk `step` of GEMM 1, else chunk step - NCH of GEMM 2
    constexpr bool RB = decltype(role_c)::value;
    const double *__restrict__ Tv = step < NCH ? T1v : T2v, *__restrict__ Tm = step < NCH ? T1m : T2m; const int ch = step < NCH ? step : step - NCH;
#pragma unroll
    for (int k = 0; k < CHK; ++k) {
#pragma unroll
      for (int f = 0; f < (RB ? NCT : 1); ++f) { const int ct = RB ? f : fixed; tf[buf][0][k][f] = Tv[((int64_t)ct * KK + CHK * ch + k) * 64]; tf[buf][1][k][f] = Tm[((int64_t)ct * KK + CHK * ch + k) * 64]; }
    }
  };
  v4d accv[NACC], accm[NACC];
  auto zero_acc = [&]() {
#pragma unroll
    for (int t = 0; t < NACC; ++t) { accv[t] = v4d{0, 0, 0, 0}; accm[t] = v4d{0, 0, 0, 0}; }
  };
  // contract columns: tile (bt, ct) = sum_k data(rows of batch tile bt, k) T(rows of class tile ct, k); contract rows: tile (ct, bt) = sum_k T(rows of class tile ct, k) data(k, columns of batch tile bt);
  // k runs over the class region (offset H for the midpoint class), whole trailing k-steps are skipped (wave-uniform)
  auto gemm = [&](auto role_c, auto contract_cols, auto ld_c, auto first_step_c, int kkv, int kkm) {
    constexpr bool RB = decltype(role_c)::value, kCols = decltype(contract_cols)::value; constexpr int LD = decltype(ld_c)::value, S0 = decltype(first_step_c)::value;
    constexpr int ND = RB ? 1 : NA, NF = RB ? NCT : 1;          // data fragments / transform fragments per class and k-step
    const double *La = (kCols ? L + j * LD + kq : L + kq * LD + j) + (RB ? (kCols ? 16 * fixed * LD : 16 * fixed) : 0);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int buf = (S0 + kk / CHK) & 1;
#pragma unroll
      for (int cls = 0; cls < 2; ++cls) {
        if (kk < (cls ? kkm : kkv)) {
          double d[ND];
#pragma unroll
          for (int t = 0; t < ND; ++t) d[t] = kCols ? La[16 * t * LD + cls * H + 4 * kk] : La[(cls * H + 4 * kk) * LD + 16 * t];
#pragma unroll
          for (int a = 0; a < (RB ? NF : ND); ++a) {
            const double dv = d[RB ? 0 : a], tv = tf[buf][cls][kk % CHK][RB ? a : 0];
            v4d &acc = cls ? accm[a] : accv[a];
            acc = kCols ? __builtin_amdgcn_mfma_f64_16x16x4f64(dv, tv, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(tv, dv, acc, 0, 0, 0);
          }
        }
      }
      // (pass 2: GEMM 2's first chunks are requested behind the epilogue instead - held across its reciprocal sequences they cost the third wave per SIMD)
      if (kk % CHK == CHK - 1 && S0 + kk / CHK + 2 < ((MODE == 1 && S0 == 0) ? NCH : 2 * NCH)) load_chunk(role_c, buf, S0 + kk / CHK + 2);
    }
  };
  // the role is wave-uniform; both bodies are branch-free instruction streams
  auto by_role = [&](auto f) {
    if constexpr (!QUAD) f(std::false_type{});
    else if constexpr (MODE == 1) f(std::true_type{});
    else { if (roleB) f(std::true_type{}); else f(std::false_type{}); }
  };
  typedef std::integral_constant<bool, kColsFirst> CF; typedef std::integral_constant<int, LD1> L1c;
  typedef std::integral_constant<bool, kColsSecond> CS; typedef std::integral_constant<int, LD2> L2c;
  typedef std::integral_constant<int, 0> S0c; typedef std::integral_constant<int, NCH> S1c;
  by_role([&](auto r) { load_chunk(r, 0, 0); load_chunk(r, 1, 1); });
  zero_acc();
  __syncthreads();
  by_role([&](auto r) { gemm(r, CF{}, L1c{}, S0c{}, P.kkv[0], P.kkm[0]); });
  __syncthreads();                                   // everybody has finished reading the input block
  // ---- first result -> LDS in the layout of the second GEMM ----
  if constexpr (MODE == 0) {           // tile (bt, ct): (y line index 16 bt + 4 q + kq, x slot 16 ct + j): mix of x with the lane's four coefficients
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
      const int s = 16 * ct + j;
      const double *__restrict__ m1 = P.mix[0][c][p1] + 4 * s;
      const double2 w0 = *reinterpret_cast<const double2 *>(m1), w1 = *reinterpret_cast<const double2 *>(m1 + 2);
      if (s < H) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double av = accv[a][q], bb = accm[a][q]; const int row = 16 * bt + 4 * q + kq;
          L[row * LD2 + s] = fma(w0.x, av, w0.y * bb); L[row * LD2 + H + s] = fma(w1.x, av, w1.y * bb);
        }
      }
    }
  } else if constexpr (MODE == 2) {    // tile (ct, bt): (y position 16 ct + 4 q + kq, x slot region column 16 bt + j): the mixes are done
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = 16 * ct + 4 * q + kq;
        if (p < H) { L[p * LD2 + 16 * bt + j] = accv[a][q]; L[(H + p) * LD2 + 16 * bt + j] = accm[a][q]; }
      }
    }
  } else {                             // tile (ct, bt): (z slot 16 ct + 4 q + kq, column 16 bt + j): mix, divide by the eigenvalue sums, transposed mix
    const double *__restrict__ lamz = P.lam_z[c][p1], *__restrict__ m1 = P.mix[0][c][p1];
    const double *bx = P.bxy + (int64_t)(4 * c + (o & 3)) * P.pl; const double czc = P.cz[c];
    double gz = 0;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
      const double bxy = bx[min(b * P.C + 16 * bt + j, P.pl - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = 16 * ct + 4 * q + kq;
        const double2 w0 = *reinterpret_cast<const double2 *>(m1 + 4 * s), w1 = *reinterpret_cast<const double2 *>(m1 + 4 * s + 2);
        const double lzv = lamz[s], lzm = lamz[64 + s];
        const double av = accv[a][q], bb = accm[a][q];
        const double gv = fma(w0.x, av, w0.y * bb), gm = fma(w1.x, av, w1.y * bb);
        // reciprocal by v_rcp_f64 + one Newton step; modes that do not exist carry lam = inf and give exactly 0
        const double dv = fma(czc, lzv, bxy), dm = fma(czc, lzm, bxy);
        double rv = __builtin_amdgcn_rcp(dv), rm = __builtin_amdgcn_rcp(dm);
        rv = dv < 1e300 ? fma(rv, fma(-dv, rv, 1.0), rv) : 0.0; rm = dm < 1e300 ? fma(rm, fma(-dm, rm, 1.0), rm) : 0.0;
        const double zv = gv * rv, zm = gm * rm;
        if constexpr (GZ) gz = fma(gm, zm, fma(gv, zv, gz));
        if (s < H) { L[s * LD2 + 16 * bt + j] = fma(w0.x, zv, w1.x * zm); L[(H + s) * LD2 + 16 * bt + j] = fma(w0.y, zv, w1.y * zm); }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (GZ) {                 // wave sums -> LDS; the barrier in front of the second GEMM publishes them
      gz = wave_sum(gz);
      if (lane == 0) gz_wave[w] = gz;
    }
  }
  if constexpr (MODE == 1) by_role([&](auto r) { load_chunk(r, NCH & 1, NCH); load_chunk(r, (NCH + 1) & 1, NCH + 1); });
  zero_acc();
  __syncthreads();
  if constexpr (GZ) {
    if (tid == 0) { double t = 0; for (int k = 0; k < NW; ++k) t += gz_wave[k]; P.gz_part[blockIdx.x] = t; }   // fixed order: bitwise reproducible
  }
  by_role([&](auto r) { gemm(r, CS{}, L2c{}, S1c{}, P.kkv[1], P.kkm[1]); });
  // ---- store ----
  if constexpr (MODE == 0) {           // tile (ct, bt): (y slot 16 ct + 4 q + kq, x slot region column 16 bt + j): mix of y, then the compact class-major order; every entry of the plane is written, the pad column too
    const double *__restrict__ m2 = P.mix[1][c][p2];
    const int nvx = P.nvx, nvy = P.nvy, nmy = P.nmy;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
      const int cpos = 16 * bt + j, col = cpos < H ? (cpos < nvx ? cpos : -1) : (cpos - H < C - nvx ? nvx + cpos - H : -1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = 16 * ct + 4 * q + kq;
        const double2 w0 = *reinterpret_cast<const double2 *>(m2 + 4 * s), w1 = *reinterpret_cast<const double2 *>(m2 + 4 * s + 2);
        const double av = accv[a][q], bb = accm[a][q];
        if (col >= 0 && s < nvy) out[base + (int64_t)s * P.row_stride + col] = fma(w0.x, av, w0.y * bb);
        if (col >= 0 && s < nmy) out[base + (int64_t)(nvy + s) * P.row_stride + col] = fma(w1.x, av, w1.y * bb);
      }
    }
  } else if constexpr (MODE == 2) {    // tile (bt, ct): (y line index 16 bt + 4 q + kq, x position 16 ct + j): nodes 2 p and 2 p + 1 of the row in one 16-byte store
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
      const int px = 16 * ct + j;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rn = node_of(16 * bt + 4 * q + kq);
        if (px < H && rn < R && 2 * px < C) *reinterpret_cast<double2 *>(out + base + (int64_t)rn * P.row_stride + 2 * px) = double2{accv[a][q], accm[a][q]};
      }
    }
  } else {                             // tile (ct, bt): (z position 16 ct + 4 q + kq, column 16 bt + j): rows 2 p and 2 p + 1
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int ct, bt; if (!tile_of(a, ct, bt)) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = 16 * ct + 4 * q + kq, cc = 16 * bt + j;
        if (p < H && cc < C) {
          if (2 * p < R) out[base + (int64_t)(2 * p) * P.row_stride + cc] = accv[a][q];
          if (2 * p + 1 < R) out[base + (int64_t)(2 * p + 1) * P.row_stride + cc] = accm[a][q];
        }
      }
    }
  }
}

// ---- the strip form of the scalar passes (one rank, the flags of the General variant without the slab extras) ------------------------------------------------------------
// A scalar Q1 system has one block per z plane (passes 1 / 3) and a few dozen chunks (pass 2): k_fdmo_pass starts far fewer workgroups than the chip has CUs, and a launch
// lasts as long as ONE workgroup needs for its two chained GEMMs.  Here a block is shared out over NT workgroups of NT waves, one tile per wave and GEMM:
//   MODE 0 (Y = T2 (X T1^T)): workgroup (block, s) computes tile column s of the intermediate - which needs all of X - and from it tile column s of Y;
//   MODE 2 (Y = (T1 X) T2^T): likewise tile row s of the intermediate and of Y;
//   MODE 1 (independent lines): chunks of 16 columns (P.C = 16) instead of one tile column per wave, wave w owns tile row w.
// Every workgroup of a block stages the whole block (L2 hits after the first); no tile is computed twice.  Bits: a tile's accumulator sees the k-steps of its two sums in
// ascending order and skips the same trailing ones (kk1, kk2) as in k_fdmo_pass, and pass 2 scales with the same operations (`scale`), so the stored values are the same.
// Passes 1 / 3 read blocks that other workgroups of the same launch read too: NOT in place (the scalar form runs g -> t, t -> t (pass 2, own columns only), t -> z).
// No stopping test, no g . z, no stamps: the scalar passes are handed none.  A strip without valid outputs leaves at once (lines much shorter than the longest direction's)
template <int NT, int MODE>
__global__ void __launch_bounds__(64 * NT)
k_fdmo_strip(OctPass P, const double *in, double *out) {
  typedef PassGeom<NT> Gm;
  constexpr bool kColsFirst = MODE == 0, kColsSecond = MODE == 2;
  constexpr int LD1 = MODE == 1 ? 16 : (kColsFirst ? Gm::LDA : Gm::LDB), LD2 = MODE == 1 ? 16 : (kColsSecond ? Gm::LDA : Gm::LDB);   // (LD = 16: the B role's 16 (mod 32), PassGeom)
  constexpr int PADC = MODE == 1 ? 16 : Gm::PADN, KKP = Gm::KKP;
  extern __shared__ double L[];                              // PADN x LDMAX doubles (MODE 1: PADN x 16)
  if (pcg_gate_closed(P.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int item = MODE == 1 ? (int)blockIdx.x : (int)blockIdx.x / NT, s = MODE == 1 ? 0 : (int)blockIdx.x - item * NT;
  const int co = item / P.nblk, b = item - co * P.nblk;      // co = right-hand side (no parity parts: no_shift = 0)
  const int R = P.R, C = MODE == 1 ? min(P.C, P.pl - b * P.C) : P.C;
  if ((MODE == 0 && 16 * s >= C) || (MODE == 2 && 16 * s >= R)) return;       // (workgroup-uniform, before any barrier)
  const int64_t base = (int64_t)co * P.co_stride + (int64_t)b * P.blk_stride;
  const int64_t base_in = P.use_in_off ? (int64_t)b * P.blk_stride : base, base_out = P.use_out_off ? (int64_t)b * P.blk_stride : base;
  if (P.use_in_off) in = P.in_blk[co];
  if (P.use_out_off) out = P.out_blk[co];
  const int f1 = MODE == 1 ? w : s;                          // tile row of T1 this wave multiplies with (T2: always w)
  const double *__restrict__ T1 = static_cast<const double *>(P.T1[co][0]) + (int64_t)f1 * KKP * 64 + lane, *__restrict__ T2 = static_cast<const double *>(P.T2[co][0]) + (int64_t)w * KKP * 64 + lane;
  // all fragments of GEMM 1 and the block are requested at once, those of GEMM 2 behind the LDS stores: one memory latency in front of each GEMM at most
  double t1[KKP], t2[KKP];
#pragma unroll
  for (int kk = 0; kk < KKP; ++kk) t1[kk] = T1[kk * 64];
  {
    constexpr int TOT = Gm::PADN * PADC, PER = TOT / (64 * NT);      // (16 NT x 16 NT or 16 NT x 16 entries: a multiple of the 64 NT threads)
    static_assert(TOT % (64 * NT) == 0, "staging loop");
    double stage[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NT, r = e / PADC, cc = e - r * PADC; stage[u] = (r < R && cc < C) ? in[base_in + (int64_t)r * P.row_stride + cc] : 0.0; }
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NT, r = e / PADC, cc = e - r * PADC; L[r * LD1 + cc] = stage[u]; }
  }
#pragma unroll
  for (int kk = 0; kk < KKP; ++kk) t2[kk] = T2[kk * 64];
  __syncthreads();
  v4d acc = v4d{0, 0, 0, 0};
  {
    const double *La = kColsFirst ? L + (16 * w + j) * LD1 + kq : L + kq * LD1 + (MODE == 1 ? 0 : 16 * w) + j;
#pragma unroll
    for (int kk = 0; kk < KKP; ++kk) {
      if (kk < KKP - 3 || kk < P.kk1) {                      // (as in k_fdmo_pass: only whole trailing k-steps are skipped)
        const double d = kColsFirst ? La[4 * kk] : La[4 * kk * LD1];
        acc = kColsFirst ? __builtin_amdgcn_mfma_f64_16x16x4f64(d, t1[kk], acc, 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(t1[kk], d, acc, 0, 0, 0);
      }
    }
  }
  __syncthreads();                                           // everybody has finished reading the input block
  {
    const int tr = MODE == 2 ? s : w, tc = MODE == 0 ? s : (MODE == 2 ? w : 0);
    if constexpr (MODE == 1) {
      const double *lamz = P.lam_z[co][0]; const double czc = P.cz[co];
      const double bxy = P.bxy[min(b * P.C + j, P.pl - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // (one fused multiply-add: what the compiler makes of `czc * lam + bxy` in every instantiation of k_fdmo_pass - the assembly of both is on record, profiles/q1_strips_isa.txt)
        const double den = fma(czc, lamz[16 * w + 4 * q + kq], bxy);
        double r = __builtin_amdgcn_rcp(den);
        r = den < 1e300 ? fma(r, fma(-den, r, 1.0), r) : 0.0;
        L[(16 * tr + 4 * q + kq) * LD2 + 16 * tc + j] = acc[q] * r;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) L[(16 * tr + 4 * q + kq) * LD2 + 16 * tc + j] = acc[q];
    }
  }
  acc = v4d{0, 0, 0, 0};
  __syncthreads();
  {
    const double *La = kColsSecond ? L + (16 * s + j) * LD2 + kq : L + kq * LD2 + 16 * s + j;      // (MODE 1: s = 0)
#pragma unroll
    for (int kk = 0; kk < KKP; ++kk) {
      if (kk < KKP - 3 || kk < P.kk2) {
        const double d = kColsSecond ? La[4 * kk] : La[4 * kk * LD2];
        acc = kColsSecond ? __builtin_amdgcn_mfma_f64_16x16x4f64(d, t2[kk], acc, 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(t2[kk], d, acc, 0, 0, 0);
      }
    }
  }
  {
    const int tr = MODE == 2 ? s : w, tc = MODE == 0 ? s : (MODE == 2 ? w : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * tr + 4 * q + kq, cc = 16 * tc + j;
      if (r < R && cc < C) out[base_out + (int64_t)r * P.row_stride + cc] = acc[q];
    }
  }
}


// ---- the transform pass with fp32 transforms (opt-in: poro_ctx_set_fdm_precision, PORO_FDM_FP32) ---------------------------------------------------------------------
// The single-rank octant form only (VAR = 0 of k_fdmo_pass: 24 blocks, aligned rows, no exchange buffer), with the same workgroup shapes, tile ownership, fragment streams
// and chunking, on v_mfma_f32_16x16x4_f32.  A kernel of its own rather than a compute-type parameter of k_fdmo_pass: as a parameter it moved the register allocation of
// eight fp64 instantiations by 2-4 VGPRs, and the fp64 path is to stay what it was.
//   pass 1 (MODE 0) reads the fp64 octant array g and converts on the way into LDS; it stores FLOATS into the scratch array (reinterpreted, same indices: half of it is used);
//   pass 2 (MODE 1) reads and writes floats, in place; between its GEMMs it multiplies by an fp32 reciprocal of the fp64 eigenvalue sum;
//   pass 3 (MODE 2) reads floats and stores the fp64 octant array z.
// Rows of the float array start at even indices (even pitch, even chunk offsets): 8-byte aligned, float2 accesses - for odd and even half lines alike (hxp padding).
// The MFMA takes one A and one B value per lane exactly as the fp64 one (A[l & 15][l >> 4], B[l >> 4][l & 15]), but its four accumulators are the rows 4 kq + q of column j
// (fp64: 4 q + kq): `arow`.  Its dependent latency (40 cycles) exceeds its issue slot (32); every wave carries >= 4 independent accumulators at NT >= 4 and the accumulator
// loop is innermost, as in the fp64 kernel.  Padding: converted zeros are zeros; removed modes (lam = inf) give exactly 0 as in fp64 (guard on the fp64 sum).
// GZ: g . z in fp64 from the fp32 values the pass holds - ghat and the rounded ghat / den it stores; they have the same sign, so every term is >= 0.
// Range: |g| and |g| / den must be fp32-normal (include/poroel_hip.h).
// Here pass 3 is the first writer of z, and it stores every entry of it, pad column included (C = the row pitch; the pad rows of the float matrices are zero, the float
// intermediate is finite): z may hold anything before - it doubles as the operator's output h (ctx.hip: solve_u_fdm).
template <int NT, int MODE, bool GZ = false>
__global__ void __launch_bounds__(64 * pass_waves<NT>())
k_fdmo_pass_f32(OctPass P, const double *in, double *out) {
  static_assert(!GZ || MODE == 1, "g . z comes out of pass 2");
  typedef PassGeom<NT> Gm;
  constexpr int NW = pass_waves<NT>();
  constexpr bool EXTRA = NT > NW;
  constexpr int XT = NT - 1;
  constexpr int NL = (MODE == 1 && EXTRA) ? NW : NT;
  constexpr bool CORNER = EXTRA && MODE != 1;
  constexpr int NACC = NL + (EXTRA ? 1 : 0) + (CORNER ? 1 : 0);
  constexpr bool kColsFirst = MODE == 0, kColsSecond = MODE == 2;
  constexpr int LD1 = kColsFirst ? Gm::LDA : Gm::LDB, LD2 = kColsSecond ? Gm::LDA : Gm::LDB;
  constexpr int NS = EXTRA ? 2 : 1;
  constexpr int PADC = 16 * NL;
  extern __shared__ float Lf[];                              // PADN x LDMAX floats (dynamic: more than 64 KB at NT = 8 only)
  __shared__ double gz_wave[GZ ? NW : 1];
  // pass 1 as the first kernel of a preconditioner call inside PCG: the iteration's stopping test (PcgStopTest).  It replaces the read of `stop`, which workgroup 0 of this
  // very launch writes.  Its inputs are requested in front of the gate's own loads, so that the two latencies overlap, and the decision falls before the block is staged:
  // the test's registers are free again by then (held across the staging loads they cost the five-tile pass its third resident workgroup)
  // (four-wave workgroups: a quarter of the sum per wave, as in k_fdmo_pass)
  constexpr bool QUARTERS = MODE == 0 && NW == 4;
  __shared__ double stop_wave[QUARTERS ? 4 : 1];
  [[maybe_unused]] PcgStopQuarter stop_q; [[maybe_unused]] bool stop_pending = false;
  if (MODE == 0 && P.stop.gg_part) {
    if (QUARTERS && !P.stop.per_wave) {
      if (P.gate && (P.gate->done | P.gate->finishing)) return;
      pcg_stop_load_quarter(P.stop, stop_q); stop_pending = true;
    } else {
      PcgStopInputs stop_in;
      pcg_stop_load(P.stop, stop_in);
      if (P.gate && (P.gate->done | P.gate->finishing)) return;
      if (pcg_stop_decide(P.stop, stop_in)) return;
    }
  } else if (pcg_gate_closed(P.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  auto arow = [&](int q) { return 4 * kq + q; };             // row of accumulator register q inside its tile
  const int co = blockIdx.x / P.nblk, b = blockIdx.x % P.nblk, c = co >> 3, o = co & 7;
  const int64_t base = (int64_t)co * P.co_stride + (int64_t)b * P.blk_stride;
  const bool heavy = CORNER && w == (int)(blockIdx.x & (NW - 1));
  const int R = P.R, C = MODE == 1 ? min(P.C, P.pl - b * P.C) : P.C;
  const float *__restrict__ T1 = static_cast<const float *>(P.T1[c][(o >> P.bit1) & 1]) + lane, *__restrict__ T2 = static_cast<const float *>(P.T2[c][(o >> P.bit2) & 1]) + lane;
  const float *inf = reinterpret_cast<const float *>(in); float *outf = reinterpret_cast<float *>(out);
  // ---- block -> LDS, zero padded to PADN x PADC; all loads in flight before the first LDS store ----
  {
    constexpr int HP = PADC / 2, TOT = Gm::PADN * HP, PER = (TOT + 64 * NW - 1) / (64 * NW);
    float2 stage[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP);
      const bool ok = e < TOT && r < R && c2 < C; const int64_t at = base + (int64_t)r * P.row_stride + c2;      // (even: base, row_stride and c2 are)
      if constexpr (MODE == 0) { const double2 v = ok ? *reinterpret_cast<const double2 *>(in + at) : double2{0.0, 0.0}; stage[u] = float2{(float)v.x, (float)v.y}; }
      else stage[u] = ok ? *reinterpret_cast<const float2 *>(inf + at) : float2{0.f, 0.f};
    }
    if constexpr (QUARTERS) { if (stop_pending) pcg_stop_post_quarter(stop_q, stop_wave); }
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP); if (e < TOT) *reinterpret_cast<float2 *>(&Lf[r * LD1 + c2]) = stage[u]; }
  }
  constexpr int CHK = EXTRA ? 2 : 4, NCH = Gm::KKP / CHK;
  float tf[2][NS][CHK];
  auto load_chunk = [&](int buf, int step) {
    const float *__restrict__ T = step < NCH ? T1 : T2; const int ch = step < NCH ? step : step - NCH;
#pragma unroll
    for (int k = 0; k < CHK; ++k) {
      tf[buf][0][k] = T[((int64_t)w * Gm::KKP + CHK * ch + k) * 64];
      if constexpr (EXTRA) tf[buf][1][k] = T[((int64_t)XT * Gm::KKP + CHK * ch + k) * 64];
    }
  };
  v4f acc[NACC];
  auto zero_acc = [&]() {
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = v4f{0, 0, 0, 0};
  };
  // (tile ownership as in k_fdmo_pass)
  auto gemm = [&](auto contract_cols, auto ld_c, auto first_step_c, auto corner_c, int kk_n) {
    constexpr bool kCols = decltype(contract_cols)::value, kCorner = decltype(corner_c)::value; constexpr int LD = decltype(ld_c)::value, S0 = decltype(first_step_c)::value;
    const float *La = kCols ? Lf + j * LD + kq : Lf + kq * LD + j;
    const float *Lw = kCols ? La + 16 * w * LD : La + 16 * w;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int buf = (S0 + ch) & 1;
#pragma unroll
      for (int k = 0; k < CHK; ++k) {
        const int kk = CHK * ch + k;
        if (kk < Gm::KKP - 3 || kk < kk_n) {
          float d[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) if (t < NL || (kCorner && t == XT)) d[t] = kCols ? La[16 * t * LD + 4 * kk] : La[4 * kk * LD + 16 * t];
          float dw = 0; if constexpr (EXTRA) dw = kCols ? Lw[4 * kk] : Lw[4 * kk * LD];
#pragma unroll
          for (int t = 0; t < NL; ++t) acc[t] = kCols ? __builtin_amdgcn_mfma_f32_16x16x4f32(d[t], tf[buf][0][k], acc[t], 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(tf[buf][0][k], d[t], acc[t], 0, 0, 0);
          if constexpr (EXTRA) acc[NL] = kCols ? __builtin_amdgcn_mfma_f32_16x16x4f32(dw, tf[buf][1][k], acc[NL], 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(tf[buf][1][k], dw, acc[NL], 0, 0, 0);
          if constexpr (kCorner) acc[NL + 1] = kCols ? __builtin_amdgcn_mfma_f32_16x16x4f32(d[XT], tf[buf][1][k], acc[NL + 1], 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(tf[buf][1][k], d[XT], acc[NL + 1], 0, 0, 0);
        }
      }
      if (S0 + ch + 2 < 2 * NCH) load_chunk(buf, S0 + ch + 2);
    }
  };
  auto tile_of = [&](int a, int &tr, int &tc, bool cols) {
    if (a < NL) { tr = cols ? a : w; tc = cols ? w : a; }
    else if (a == NL) { tr = cols ? w : XT; tc = cols ? XT : w; }
    else { tr = XT; tc = XT; }
  };
  typedef std::integral_constant<bool, kColsFirst> CF; typedef std::integral_constant<int, LD1> L1c;
  typedef std::integral_constant<bool, kColsSecond> CS; typedef std::integral_constant<int, LD2> L2c;
  typedef std::integral_constant<int, 0> S0c; typedef std::integral_constant<int, NCH> S1c;
  __builtin_amdgcn_s_setprio(3);
  load_chunk(0, 0); load_chunk(1, 1);
  zero_acc();
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();
  if constexpr (QUARTERS) { if (stop_pending && pcg_stop_decide_quarters(P.stop, stop_q, stop_wave)) return; }
  if (heavy) gemm(CF{}, L1c{}, S0c{}, std::integral_constant<bool, CORNER>{}, P.kk1); else gemm(CF{}, L1c{}, S0c{}, std::false_type{}, P.kk1);
  __syncthreads();
  // ---- first result -> LDS in the layout of the second GEMM (MODE 1: divided by the eigenvalue sums on the way) ----
  if constexpr (MODE == 1) {
    const double *lamz = P.lam_z[c][(o >> 2) & 1], *bx = P.bxy + (int64_t)(4 * c + (o & 3)) * P.pl;
    const double czc = P.cz[c];
    double lzw[4], lzx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { lzw[q] = czc * lamz[16 * w + arow(q)]; lzx[q] = EXTRA ? czc * lamz[16 * XT + arow(q)] : 0.0; }
    double gz = 0;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int tr, tc; tile_of(a, tr, tc, false);
      const double bxy = bx[min(b * P.C + 16 * tc + j, P.pl - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // the fp64 eigenvalue sum, rounded once, then v_rcp_f32 (1 ulp); modes that do not exist (lam = inf) and sums beyond the fp32 range give exactly 0
        const double den = (a < NL ? lzw[q] : lzx[q]) + bxy;
        const float r = den < 1e300 ? __builtin_amdgcn_rcpf((float)den) : 0.f;
        const float zh = acc[a][q] * r;
        Lf[(16 * tr + arow(q)) * LD2 + 16 * tc + j] = zh;
        if constexpr (GZ) gz = fma((double)acc[a][q], (double)zh, gz);
        __builtin_amdgcn_sched_barrier(0);       // one entry at a time, as in k_fdmo_pass: otherwise the conversions and reciprocals of all entries pile up in registers
      }
    }
    if constexpr (GZ) {
      gz = wave_sum(gz);
      if (lane == 0) gz_wave[w] = gz;
    }
  } else {
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      int tr, tc; tile_of(a, tr, tc, kColsFirst);
      if (a == NL + 1 && !heavy) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) Lf[(16 * tr + arow(q)) * LD2 + 16 * tc + j] = acc[a][q];
    }
  }
  zero_acc();
  __syncthreads();
  if constexpr (GZ) {
    if (tid == 0) { double t = 0; for (int k = 0; k < NW; ++k) t += gz_wave[k]; P.gz_part[blockIdx.x] = t; }   // fixed order: reproducible
  }
  if (heavy) gemm(CS{}, L2c{}, S1c{}, std::integral_constant<bool, CORNER>{}, P.kk2); else gemm(CS{}, L2c{}, S1c{}, std::false_type{}, P.kk2);
  // ---- store: floats (passes 1, 2) or the fp64 octant array (pass 3) ----
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    int tr, tc; tile_of(a, tr, tc, kColsSecond);
    if (a == NL + 1 && !heavy) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * tr + arow(q), cc = 16 * tc + j;
      if (r < R && cc < C) { const int64_t at = base + (int64_t)r * P.row_stride + cc; if constexpr (MODE == 2) out[at] = (double)acc[a][q]; else outf[at] = acc[a][q]; }
    }
  }
}

// ---- planar (2D) form: the blocks are whole (component, quadrant) planes of up to ~350 x 350 entries - too large for one workgroup's LDS, so each of the four
//      1D transforms is a batched tiled GEMM of its own: C_b (M x N) = A_b (M x K) B_b (K x N), 64 x 64 tiles, 16-deep LDS stages (double buffered), 4 waves x (2 x 2) MFMA tiles.
//      An operand whose unit stride runs along K is staged "m-major" ([64][16 + 2]), one whose unit stride runs along M / N "k-major" ([16][64 + 16]): both give
//      conflict-free fragment reads (ds_read_b64: 32 lanes per cycle on 32 bank pairs) and contiguous global loads ----
struct Gemm2D {
  int M, N, K, nb;
  int64_t rsA, csA, rsB, csB, rsC;       // element strides (C: unit column stride)
  const double *A[8], *B[8]; double *C[8];   // per batch entry
  int scale; const double *lamM[8], *lamN[8]; double cM[8], cN[8];   // epilogue: C[m][n] /= cM lamM[m] + cN lamN[n] (inf -> 0)
  const PcgScalars *gate;
  PcgStopTest stop;      // the first GEMM of a preconditioner call inside PCG: the iteration's stopping test (common.hpp); gg_part == null elsewhere
};
template <bool KCONTIG> struct GemmLds { static constexpr int LD = KCONTIG ? 18 : 80, SIZE = KCONTIG ? 64 * 18 : 16 * 80; };
template <bool AK, bool BK>
__global__ void __launch_bounds__(256) k_fdmo_gemm2d(Gemm2D G) {
  typedef GemmLds<AK> LA; typedef GemmLds<BK> LB;
  __shared__ double As[2][LA::SIZE], Bs[2][LB::SIZE];
  if (G.stop.gg_part) {
    if (G.gate && (G.gate->done | G.gate->finishing)) return;
    if (pcg_stop_test(G.stop)) return;
  } else if (pcg_gate_closed(G.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, j = lane & 15, kq = lane >> 4;
  const int tiles_n = (G.N + 63) / 64, tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n, b = blockIdx.y;
  const int m0 = 64 * tm, n0 = 64 * tn;
  const double *__restrict__ Ab = G.A[b], *__restrict__ Bb = G.B[b];
  // global -> registers: 4 consecutive elements along the operand's unit-stride direction per thread
  double ra[4], rb[4];
  auto gload = [&](int k0) {
    if (AK) { const int m = m0 + (tid >> 2), k = k0 + 4 * (tid & 3);
#pragma unroll
      for (int u = 0; u < 4; ++u) ra[u] = (m < G.M && k + u < G.K) ? Ab[(int64_t)m * G.rsA + (int64_t)(k + u) * G.csA] : 0.0; }
    else { const int k = k0 + (tid >> 4), m = m0 + 4 * (tid & 15);
#pragma unroll
      for (int u = 0; u < 4; ++u) ra[u] = (k < G.K && m + u < G.M) ? Ab[(int64_t)(m + u) * G.rsA + (int64_t)k * G.csA] : 0.0; }
    if (BK) { const int n = n0 + (tid >> 2), k = k0 + 4 * (tid & 3);
#pragma unroll
      for (int u = 0; u < 4; ++u) rb[u] = (n < G.N && k + u < G.K) ? Bb[(int64_t)(k + u) * G.rsB + (int64_t)n * G.csB] : 0.0; }
    else { const int k = k0 + (tid >> 4), n = n0 + 4 * (tid & 15);
#pragma unroll
      for (int u = 0; u < 4; ++u) rb[u] = (k < G.K && n + u < G.N) ? Bb[(int64_t)k * G.rsB + (int64_t)(n + u) * G.csB] : 0.0; }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (AK) As[buf][(tid >> 2) * LA::LD + 4 * (tid & 3) + u] = ra[u]; else As[buf][(tid >> 4) * LA::LD + 4 * (tid & 15) + u] = ra[u];
      if (BK) Bs[buf][(tid >> 2) * LB::LD + 4 * (tid & 3) + u] = rb[u]; else Bs[buf][(tid >> 4) * LB::LD + 4 * (tid & 15) + u] = rb[u];
    }
  };
  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) for (int c = 0; c < 2; ++c) acc[a][c] = v4d{0, 0, 0, 0};
  const int nk = (G.K + 15) / 16;
  gload(0); lstore(0);
  __syncthreads();
  for (int s = 0; s < nk; ++s) {
    const int buf = s & 1;
    if (s + 1 < nk) gload(16 * (s + 1));
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) { const int m = 32 * wm + 16 * a + j, k = 4 * kk + kq; fa[a] = AK ? As[buf][m * LA::LD + k] : As[buf][k * LA::LD + m]; }
#pragma unroll
      for (int c = 0; c < 2; ++c) { const int n = 32 * wn + 16 * c + j, k = 4 * kk + kq; fb[c] = BK ? Bs[buf][n * LB::LD + k] : Bs[buf][k * LB::LD + n]; }
#pragma unroll
      for (int a = 0; a < 2; ++a) for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
    }
    if (s + 1 < nk) lstore(buf ^ 1);       // (the other buffer: everybody finished reading it before the barrier that ended the previous stage)
    __syncthreads();
  }
  double *__restrict__ Cb = G.C[b];
#pragma unroll
  for (int a = 0; a < 2; ++a) for (int c = 0; c < 2; ++c) {
    const int col = n0 + 32 * wn + 16 * c + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = m0 + 32 * wm + 16 * a + 4 * q + kq;
      if (row < G.M && col < G.N) {
        double v = acc[a][c][q];
        if (G.scale) { const double den = G.cM[b] * G.lamM[b][row] + G.cN[b] * G.lamN[b][col]; v = den < 1e300 ? v / den : 0.0; }
        Cb[(int64_t)row * G.rsC + col] = v;
      }
    }
  }
}

// ---- slab form, z stage with BOTH parity parts of a line in one workgroup (NT = 2, 4, 5) --------------------------------------------------------------------------
// A workgroup takes 8 NL real columns of the rank's share: it loads every gathered plane ONCE, forms the even part e_k = v_k + v_k' into the left half of the LDS
// block and the odd part o_k = v_k - v_k' into the right half, runs the half-size forward / scale / backward chain on both halves at once (the column tiles of the
// left half use the even-mode matrices, those of the right half the odd-mode ones: two fragment streams per wave, + one for the shared tile row at NT = 5), and
// stores v_k = a + b, v_k' = a - b straight into the scattering all-to-all's buffer - every plane to the one or two ranks that hold it (dst table).  Replaces the
// two-workgroups-per-chunk pass (each parity read every plane pair again) and the separate scatter kernel.
template <int NT>
__global__ void __launch_bounds__(64 * (NT < 4 ? NT : 4))
k_fdmo_zpass_both(OctPass P, const int64_t *__restrict__ dst /* [ng][2]: offsets of a plane's rows in the exchange buffer, -1 = none */, const double *in, double *out) {
  typedef PassGeom<NT> Gm;
  constexpr int NW = NT < 4 ? NT : 4; constexpr bool EXTRA = NT > NW; constexpr int XT = NT - 1;
  constexpr int NL = NW, HT = NL / 2, HC = 16 * HT;            // column tiles of the LDS block (left half: even part, right half: odd part), real columns of a chunk
  static_assert(NL % 2 == 0, "both-parity z pass: an even number of column tiles");
  constexpr int LD = Gm::LDB, NACC = NL + (EXTRA ? 1 : 0), NS = EXTRA ? 3 : 2;
  __shared__ double L[Gm::PADN * Gm::LDB];
  if (P.gate && (P.gate->done | P.gate->finishing)) return;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 15, kq = lane >> 4;
  const int G = P.chunk0 + (int)blockIdx.x, cq = G / P.nchunk;
  if (G >= P.chunk_total) return;
  const int b = G - cq * P.nchunk, c = cq >> 2, qd = cq & 3;
  const int R = P.R, C = min(HC, P.pl - b * HC);
  const int pw = w >= HT ? 1 : 0;                              // parity of the column tile this wave's share of the extra tile row belongs to
  const int64_t cb = (int64_t)blockIdx.x * HC;                 // first column of the chunk inside the rank's share
  // ---- gathered planes -> parity parts in LDS ----
  {
    constexpr int HP = HC / 2, TOT = Gm::PADN * HP, PER = (TOT + 64 * NW - 1) / (64 * NW);
    double2 lo[PER], hi[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP);
      const bool ok = e < TOT && r < R && c2 < C; const int rr = ok ? r : 0, mr = P.ng - 1 - rr;
      lo[u] = ok ? *reinterpret_cast<const double2 *>(in + P.row_in[rr] + cb + c2) : double2{0.0, 0.0};
      hi[u] = (ok && mr != rr) ? *reinterpret_cast<const double2 *>(in + P.row_in[mr] + cb + c2) : double2{0.0, 0.0};
      if (ok && mr == rr) hi[u] = double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * NW, r = e / HP, c2 = 2 * (e - r * HP);
      if (e < TOT) {
        const bool centre = r < R && (P.ng - 1 - r) == r;
        *reinterpret_cast<double2 *>(&L[r * LD + c2]) = double2{lo[u].x + hi[u].x, lo[u].y + hi[u].y};
        *reinterpret_cast<double2 *>(&L[r * LD + HC + c2]) = centre ? double2{0.0, 0.0} : double2{lo[u].x - hi[u].x, lo[u].y - hi[u].y};
      }
    }
  }
  constexpr int CHK = 2, NCH = Gm::KKP / CHK;
  double tf[2][NS][CHK];
  const double *__restrict__ T1e = static_cast<const double *>(P.T1[c][0]) + lane, *__restrict__ T1o = static_cast<const double *>(P.T1[c][1]) + lane, *__restrict__ T2e = static_cast<const double *>(P.T2[c][0]) + lane, *__restrict__ T2o = static_cast<const double *>(P.T2[c][1]) + lane;
  auto load_chunk = [&](int buf, int step) {
    const bool first = step < NCH; const int ch = first ? step : step - NCH;
    const double *__restrict__ Te = first ? T1e : T2e, *__restrict__ To = first ? T1o : T2o;
#pragma unroll
    for (int k = 0; k < CHK; ++k) {
      tf[buf][0][k] = Te[((int64_t)w * Gm::KKP + CHK * ch + k) * 64];
      tf[buf][1][k] = To[((int64_t)w * Gm::KKP + CHK * ch + k) * 64];
      if constexpr (EXTRA) tf[buf][2][k] = (pw ? To : Te)[((int64_t)XT * Gm::KKP + CHK * ch + k) * 64];
    }
  };
  v4d acc[NACC];
  auto zero_acc = [&]() {
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = v4d{0, 0, 0, 0};
  };
  // acc[u] = tile (w, u) = sum_k T_par(u)(rows of tile w, k) data(k, columns of tile u); extra: acc[NL] = tile (XT, w)
  auto gemm = [&](auto first_step_c, int kk_n) {
    constexpr int S0 = decltype(first_step_c)::value;
    const double *La = L + kq * LD + j, *Lw = La + 16 * w;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int buf = (S0 + ch) & 1;
#pragma unroll
      for (int k = 0; k < CHK; ++k) {
        const int kk = CHK * ch + k;
        if (kk < Gm::KKP - 3 || kk < kk_n) {
          double d[NL];
#pragma unroll
          for (int t = 0; t < NL; ++t) d[t] = La[4 * kk * LD + 16 * t];
          double dw = 0; if constexpr (EXTRA) dw = Lw[4 * kk * LD];
#pragma unroll
          for (int t = 0; t < NL; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(tf[buf][t < HT ? 0 : 1][k], d[t], acc[t], 0, 0, 0);
          if constexpr (EXTRA) acc[NL] = __builtin_amdgcn_mfma_f64_16x16x4f64(tf[buf][2][k], dw, acc[NL], 0, 0, 0);
        }
      }
      if (S0 + ch + 2 < 2 * NCH) load_chunk(buf, S0 + ch + 2);
    }
  };
  __builtin_amdgcn_s_setprio(3);
  load_chunk(0, 0); load_chunk(1, 1);
  zero_acc();
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();
  gemm(std::integral_constant<int, 0>{}, P.kk1);
  __syncthreads();
  // ---- divided by the eigenvalue sums -> LDS (same layout) ----
  {
    const double *bx = P.bxy + (int64_t)(4 * c + qd) * P.pl; const double czc = P.cz[c];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      const int tr = a < NL ? w : XT, tc = a < NL ? a : w, par = tc >= HT ? 1 : 0;
      const double *lamz = P.lam_z[c][par];
      const double bxy = bx[min(b * HC + 16 * (tc - par * HT) + j, P.pl - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double den = fma(czc, lamz[16 * tr + 4 * q + kq], bxy);
        double r = __builtin_amdgcn_rcp(den);
        r = den < 1e300 ? fma(r, fma(-den, r, 1.0), r) : 0.0;
        L[(16 * tr + 4 * q + kq) * LD + 16 * tc + j] = acc[a][q] * r;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  zero_acc();
  __syncthreads();
  gemm(std::integral_constant<int, NCH>{}, P.kk2);
  // ---- v_k = a + b, v_k' = a - b -> the scattering all-to-all's buffer ----
  auto put = [&](int row, int col, double a, double bb) {
    if (row >= R || col >= C) return;
    const int mr = P.ng - 1 - row;
    const double vlo = mr == row ? a : a + bb, vhi = a - bb;
#pragma unroll
    for (int t = 0; t < 2; ++t) { const int64_t d0 = dst[2 * row + t]; if (d0 >= 0) out[d0 + cb + col] = vlo; }
    if (mr != row) {
#pragma unroll
      for (int t = 0; t < 2; ++t) { const int64_t d1 = dst[2 * mr + t]; if (d1 >= 0) out[d1 + cb + col] = vhi; }
    }
  };
#pragma unroll
  for (int u = 0; u < HT; ++u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) put(16 * w + 4 * q + kq, 16 * u + j, acc[u][q], acc[u + HT][q]);
  }
  if constexpr (EXTRA) {
    // the shared tile row: waves 0 .. HT-1 hold the even-mode sums of column tile w, waves HT .. hold the odd-mode sums of column tile w - HT: swap through LDS
    __syncthreads();                                 // (everybody has finished reading the block)
    if (pw) {
#pragma unroll
      for (int q = 0; q < 4; ++q) L[((w - HT) * 4 + q) * 64 + lane] = acc[NL][q];
    }
    __syncthreads();
    if (!pw) {
#pragma unroll
      for (int q = 0; q < 4; ++q) put(16 * XT + 4 * q + kq, 16 * w + j, acc[NL][q], L[(w * 4 + q) * 64 + lane]);
    }
  }
}
template <int NT> void launch_zpass_both(hipStream_t s, const OctPass &P, const int64_t *dst, int n_items, const double *in, double *out, hipEvent_t e0, hipEvent_t e1) {
  hipExtLaunchKernelGGL((k_fdmo_zpass_both<NT>), dim3((unsigned)n_items), dim3(64 * (NT < 4 ? NT : 4)), 0, s, e0, e1, 0, P, dst, in, out);
}

// one instantiation: dynamic LDS of PADN x LDMAX elements (more than 64 KB from NT = 6 on in fp64: opted in once per device and instantiation), events attached to the
// dispatch itself (the kernel's own duration, as rocprofv3 reports it)
template <auto Kernel, int NT, class Elem> void launch_one(hipStream_t s, int n_items, const OctPass &P, const double *in, double *out, hipEvent_t e0, hipEvent_t e1) {
  constexpr unsigned lds = (unsigned)(PassGeom<NT>::PADN * PassGeom<NT>::LDMAX * sizeof(Elem));
  if (lds > 64 * 1024) {
    static std::mutex mu; static std::set<int> done; int dev = 0; PORO_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (!done.count(dev)) { PORO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); done.insert(dev); }
  }
  hipExtLaunchKernelGGL(Kernel, dim3((unsigned)n_items), dim3(64 * pass_waves<NT>()), lds, s, e0, e1, 0, P, in, out);
}
// The kernel variant of a pass is stated by whoever builds the descriptor.  Octant / SlabU (VAR = 0 / 1 of k_fdmo_pass) fold the flags below at compile time and never read
// them, PerDirection (VAR = 3) folds what Octant folds and reads the part geometry (OctPass::per_dir), General (VAR = 2) reads them, OctantF32 is k_fdmo_pass_f32 (float fragments in P.T1 / P.T2, float intermediate array; it folds what Octant folds)
enum class PassVariant { Octant, SlabU, General, OctantF32, PerDirection };
constexpr const char *kVariantName[] = {"Octant", "SlabU", "General", "OctantF32", "PerDirection"};
PassVariant variant_of_flags(const OctPass &P) {       // the variant whose folded switches equal the descriptor's flags
  const bool plain = P.vec2 == 1 && !P.use_in_off && !P.use_out_off && P.bxy_cmul == 4;
  const bool unit = P.vec2 == 1 && !P.use_in_off && !P.use_out_off && P.slab_z == 0 && P.slab_io == 0 && !P.row_in;
  if (P.per_dir) return unit && P.bxy_cmul >= 1 && P.bxy_cmul <= 4 && P.no_shift >= 0 && P.no_shift < 3 ? PassVariant::PerDirection : PassVariant::General;
  const bool oct = plain && P.slab_z == 0 && P.slab_io == 0 && !P.row_in && P.no_shift == 3;
  const bool slab_u = plain && P.no_shift == 2 && ((P.mode == 0 && P.slab_io == 1 && !P.slab_z) || (P.mode == 1 && P.slab_z == 2 && P.row_in && !P.slab_io) || (P.mode == 2 && P.slab_io == 2 && !P.slab_z));
  return oct ? PassVariant::Octant : slab_u ? PassVariant::SlabU : PassVariant::General;
}
template <int NT, int VAR> void launch_modes(hipStream_t s, const OctPass &P, int n_items, const double *in, double *out, hipEvent_t e0, hipEvent_t e1) {
  if (P.mode == 0) launch_one<k_fdmo_pass<NT, 0, VAR>, NT, double>(s, n_items, P, in, out, e0, e1);
  else if (P.mode == 2) launch_one<k_fdmo_pass<NT, 2, VAR>, NT, double>(s, n_items, P, in, out, e0, e1);
  else if ((VAR == 0 || VAR == 3) && P.gz_part) launch_one<k_fdmo_pass<NT, 1, (VAR == 3 ? 3 : 0), true>, NT, double>(s, n_items, P, in, out, e0, e1);
  else launch_one<k_fdmo_pass<NT, 1, VAR>, NT, double>(s, n_items, P, in, out, e0, e1);
}
template <int NT> void launch_pass(hipStream_t s, PassVariant v, const OctPass &P, int n_items, const double *in, double *out, hipEvent_t e0, hipEvent_t e1) {
  switch (v) {
    case PassVariant::Octant: launch_modes<NT, 0>(s, P, n_items, in, out, e0, e1); break;
    case PassVariant::SlabU: launch_modes<NT, 1>(s, P, n_items, in, out, e0, e1); break;
    case PassVariant::General: launch_modes<NT, 2>(s, P, n_items, in, out, e0, e1); break;
    case PassVariant::PerDirection: launch_modes<NT, 3>(s, P, n_items, in, out, e0, e1); break;
    case PassVariant::OctantF32:
      if (P.mode == 0) launch_one<k_fdmo_pass_f32<NT, 0>, NT, float>(s, n_items, P, in, out, e0, e1);
      else if (P.mode == 2) launch_one<k_fdmo_pass_f32<NT, 2>, NT, float>(s, n_items, P, in, out, e0, e1);
      else if (P.gz_part) launch_one<k_fdmo_pass_f32<NT, 1, true>, NT, float>(s, n_items, P, in, out, e0, e1);
      else launch_one<k_fdmo_pass_f32<NT, 1>, NT, float>(s, n_items, P, in, out, e0, e1);
      break;
  }
}
void launch_pass_nt(hipStream_t s, int nt, PassVariant v, const OctPass &P, int n_blocks, const double *in, double *out, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  const PassVariant flags = variant_of_flags(P);
  if (flags != (v == PassVariant::OctantF32 ? PassVariant::Octant : v)) throw Error(std::string("fdmo: pass stated as ") + kVariantName[(int)v] + ", the flags of its descriptor are those of " + kVariantName[(int)flags]);
  switch (nt) {
    case 1: launch_pass<1>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 2: launch_pass<2>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 3: launch_pass<3>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 4: launch_pass<4>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 5: launch_pass<5>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 6: launch_pass<6>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 7: launch_pass<7>(s, v, P, n_blocks, in, out, e0, e1); break;
    case 8: launch_pass<8>(s, v, P, n_blocks, in, out, e0, e1); break;
    default: throw Error("fdmo: half lines of more than 128 entries");
  }
}
// class-split passes: the same block, grid and LDS size as the dense octant pass of that tile count
template <int NT> void launch_vm(hipStream_t s, const OctPassVM &P, int n_items, const double *in, double *out, hipEvent_t e0, hipEvent_t e1) {
  constexpr unsigned lds = (unsigned)(PassGeom<NT>::PADN * PassGeom<NT>::LDMAX * sizeof(double));
  auto go = [&](auto kernel) {
    if (lds > 64 * 1024) {
      static std::mutex mu; static std::set<std::pair<int, const void *>> done; int dev = 0; PORO_HIP(hipGetDevice(&dev));
      std::lock_guard<std::mutex> lk(mu);
      if (!done.count({dev, reinterpret_cast<const void *>(kernel)})) { PORO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); done.insert({dev, reinterpret_cast<const void *>(kernel)}); }
    }
    hipExtLaunchKernelGGL(kernel, dim3((unsigned)n_items), dim3(64 * vm_waves<NT>()), lds, s, e0, e1, 0, P, in, out);
  };
  if (P.mode == 0) go(k_fdmo_pass_vm<NT, 0>); else if (P.mode == 2) go(k_fdmo_pass_vm<NT, 2>); else if (P.gz_part) go(k_fdmo_pass_vm<NT, 1, true>); else go(k_fdmo_pass_vm<NT, 1>);
}
void launch_vm_nt(hipStream_t s, int nt, const OctPassVM &P, int n_items, const double *in, double *out, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  switch (nt) {
    case 1: launch_vm<1>(s, P, n_items, in, out, e0, e1); break;
    case 2: launch_vm<2>(s, P, n_items, in, out, e0, e1); break;
    case 3: launch_vm<3>(s, P, n_items, in, out, e0, e1); break;
    case 4: launch_vm<4>(s, P, n_items, in, out, e0, e1); break;
    case 5: launch_vm<5>(s, P, n_items, in, out, e0, e1); break;
    case 6: launch_vm<6>(s, P, n_items, in, out, e0, e1); break;
    case 7: launch_vm<7>(s, P, n_items, in, out, e0, e1); break;
    case 8: launch_vm<8>(s, P, n_items, in, out, e0, e1); break;
    default: throw Error("fdmo: half lines of more than 128 entries");
  }
}
// columns of a pass-2 chunk: one 16-wide tile per wave (NT = 5: four waves)
inline int pass2_chunk(int nt) { return nt == 5 ? 64 : 16 * nt; }
inline int pass2_chunks(int pl, int nt) { return (pl + pass2_chunk(nt) - 1) / pass2_chunk(nt); }   // chunks of a plane of pl positions = workgroups of pass 2 per block (one rank)
inline int oct_grid(int64_t co, int nc = 3) { return (int)std::min<int64_t>((nc * co + kBlock - 1) / kBlock, kMaxPartials); }   // threads = positions x components, as many per thread as the partial slots demand
// split mask of a form: the per-direction form states it; octants split everything, quadrants (slabs, planar form) x and y, no = 1 nothing
inline int split_mask_of(const FdmOct &O) { return O.per_dir ? O.split_mask : O.no == 8 ? 7 : O.no == 4 ? 3 : 0; }
OctDims dims_of(const FdmOct &O) {
  OctDims D{O.n[0], O.n[1], O.n[2], O.h[0], O.h[1], O.h[2], O.hxp, O.co_stride, O.no, O.own_z, O.nc, split_mask_of(O), {}};
  for (int o = 0; o < 8; ++o) {        // bits of the split directions, packed in the order x, y, z
    int part = 0, k = 0;
    for (int d = 0; d < 3; ++d) if (D.split & (1 << d)) part |= ((o >> d) & 1) << k++;
    D.part[o] = (o & ~D.split) ? -1 : part;
  }
  return D;
}
SlabGeo geo_of(const FdmOct &O) { const auto &S = O.slab; return SlabGeo{S.cw, S.nchunk, S.cps, S.nb * S.nchunk, S.rank, S.my_chunks, S.hzg, S.ng, S.np, S.scols, (int64_t)O.hxp * O.h[1], O.co_stride}; }

// ---- the pass plan: one description of a form, one builder of the three launch descriptors ---------------------------------------------------------------------------
// A form = what the passes need to know about the arrays they sweep: `blocks` blocks of planes() z-planes of hy() rows of `pitch` entries, hx() of them transformed.  Pass 2
// takes lines of zlen() entries in chunks of cw() columns: the z lines of the blocks themselves (one rank) or blocks [zlen][cw] of the transposed array (slabs: global lines)
struct Form {
  const FdmOct &O; bool scalar, f32;   // scalar: every block = a right-hand side of one scalar Q1 system (one set of matrices); f32: the float fragments
  int pitch, blocks, no_shift;         // blocks of the arrays = components (right-hand sides) x parity parts; log2 of the parity parts
  int nc, np, vec2, bxy_cmul;          // components and parities that have matrices
  double kappa; const double *bxy;     // scalar: the z coefficient; x / y share of the eigenvalue sums
  int hx() const { return O.h[0]; } int hy() const { return O.h[1]; } int planes() const { return O.h[2]; }
  int zlen() const { return O.slab.on ? O.slab.hzg : O.h[2]; } int cw() const { return O.slab.on ? O.slab.cw : pass2_chunk(O.nt_z); }
  // (per-direction form: a whole direction has one matrix set, in parity slot 0 - listed for both parities)
  int slot(int d, int p) const { return O.per_dir && !(O.split_mask & (1 << d)) ? 0 : p; }
  int bit(int d) const { int k = 0; for (int e = 0; e < d; ++e) k += (split_mask_of(O) >> e) & 1; return k; }   // bit of a part's index that holds direction d's parity (octants: d)
  const void *fwd(int c, int d, int p) const { c = scalar ? 0 : c; p = slot(d, p); return f32 ? (const void *)O.fwd32[c][d][p].p : (const void *)O.fwd[c][d][p].p; }
  const void *bwd(int c, int d, int p) const { c = scalar ? 0 : c; p = slot(d, p); return f32 ? (const void *)O.bwd32[c][d][p].p : (const void *)O.bwd[c][d][p].p; }
  const double *lam_z(int c, int p) const { return O.lam[scalar ? 0 : c][2][slot(2, p)].p; } double cz(int c) const { return scalar ? kappa : O.coef[c][2]; }
};
// displacement system (octants on one rank, quadrants on slabs; rows padded to even length) / nb right-hand sides of the scalar Q1 system a M + kappa K (nodal layout)
// per-direction form: 2^(split directions) parts per component, 2^(split among x, y) planes of the bxy table per component
Form disp_form(const FdmOct &O, bool f32) {
  if (O.per_dir) { int ns = 0; for (int d = 0; d < 3; ++d) ns += (O.split_mask >> d) & 1; return Form{O, false, false, O.hxp, 3 * O.no, ns, 3, 2, 1, 1 << ((O.split_mask & 1) + ((O.split_mask >> 1) & 1)), 0.0, O.bxy.p}; }
  return Form{O, false, f32, O.hxp, 3 * O.no, O.slab.on ? 2 : 3, 3, 2, 1, 4, 0.0, O.bxy.p};
}
Form scalar_form(const FdmOct &O, int nb, double kappa, const double *table) { return Form{O, true, false, O.h[0], nb, 0, nb, 1, 0, 0, kappa, table}; }
// pass 1: per z-plane X[ky][kx] -> Fy (X Fx^T); pass 2: per chunk of cw columns X[kz][col] -> Bz scale (Fz X); pass 3: per z-plane X[my][mx] -> (By X) Bx^T.
// Everything but the per-call fields (gate, gz_part, in_blk / out_blk, stamps) and the slab extras (plan_slab_pass)
OctPass plan_pass(const Form &F, int pass) {
  auto ksteps = [](int n) { return (n + 3) / 4; };
  const int hx = F.hx(), hy = F.hy(), zlen = F.zlen(), cw = F.cw(), pl = F.pitch * hy; const bool first = pass == 1, transposed = F.O.slab.on;
  OctPass P{};
  if (F.O.per_dir) {        // the parity bits of a part's index are packed: only the split directions have one (a whole direction's two slots hold the same matrices - any bit will do)
    P.per_dir = 1; P.bitz = F.bit(2);
  }
  const int bx = F.O.per_dir ? F.bit(0) : 0, by = F.O.per_dir ? F.bit(1) : 1, bz = F.O.per_dir ? F.bit(2) : 2;
  P.co_stride = F.O.co_stride; P.pl = pl; P.bxy = F.bxy; P.vec2 = F.vec2; P.no_shift = F.no_shift; P.bxy_cmul = F.bxy_cmul;
  if (pass == 2) {       // (transposed: one block [zlen][cw] per workgroup instead of cw columns of a block of the array)
    P.mode = 1; P.R = zlen; P.C = cw; P.kk1 = P.kk2 = ksteps(zlen); P.bit1 = P.bit2 = bz;
    P.nblk = transposed ? 1 : pass2_chunks(pl, F.O.nt_z); P.blk_stride = transposed ? (int64_t)zlen * cw : cw; P.row_stride = transposed ? cw : pl;
  } else {
    P.mode = first ? 0 : 2; P.R = hy; P.C = F.pitch; P.kk1 = ksteps(first ? hx : hy); P.kk2 = ksteps(first ? hy : hx); P.bit1 = first ? bx : by; P.bit2 = first ? by : bx;
    P.nblk = F.planes(); P.blk_stride = pl; P.row_stride = F.pitch;
  }
  for (int c = 0; c < F.nc; ++c) {
    P.cz[c] = F.cz(c);
    for (int p = 0; p < F.np; ++p) {
      P.lam_z[c][p] = F.lam_z(c, p);
      if (pass == 1) { P.T1[c][p] = F.fwd(c, 0, p); P.T2[c][p] = F.fwd(c, 1, p); }
      else if (pass == 2) { P.T1[c][p] = F.fwd(c, 2, p); P.T2[c][p] = F.bwd(c, 2, p); }
      else { P.T1[c][p] = F.bwd(c, 1, p); P.T2[c][p] = F.bwd(c, 0, p); }
    }
  }
  return P;
}
// the class-split passes of the single-rank octant form: the dense plan's blocks and grids, the class tables of fdmo_upload_dir_classes
OctPassVM plan_vm(const FdmOct &O, const OctPass &D, int pass) {
  OctPassVM P{};
  P.mode = D.mode; P.R = D.R; P.C = D.C; P.nblk = D.nblk; P.pl = D.pl; P.co_stride = D.co_stride; P.blk_stride = D.blk_stride; P.row_stride = D.row_stride; P.bit1 = D.bit1; P.bit2 = D.bit2;
  const int dir[2] = {pass == 1 ? 0 : pass == 2 ? 2 : 1, pass == 1 ? 1 : pass == 2 ? 2 : 0}; const bool back[2] = {pass == 3, pass != 1};
  for (int g = 0; g < 2; ++g) {
    const int h = O.h[dir[g]]; P.kkv[g] = ((h + 1) / 2 + 3) / 4; P.kkm[g] = (h / 2 + 3) / 4;
    for (int c = 0; c < 3; ++c) for (int p = 0; p < 2; ++p) {
      P.Tv[g][c][p] = (back[g] ? O.cbwd : O.cfwd)[c][dir[g]][p][0].p; P.Tm[g][c][p] = (back[g] ? O.cbwd : O.cfwd)[c][dir[g]][p][1].p; P.mix[g][c][p] = O.cmix[c][dir[g]][p].p;
    }
  }
  P.nvx = (O.h[0] + 1) / 2; P.nvy = (O.h[1] + 1) / 2; P.nmy = O.h[1] / 2;
  for (int c = 0; c < 3; ++c) { P.cz[c] = O.coef[c][2]; for (int p = 0; p < 2; ++p) P.lam_z[c][p] = O.clam[c][2][p].p; }
  P.bxy = O.bxy_vm.p;
  return P;
}
// slab form: the same plan + where the pass meets the exchange buffer (see OctPass): pass 1 stores into it, pass 3 loads from it, pass 2 gathers whole lines from it
OctPass plan_slab_pass(const Form &F, int pass) {
  const auto &S = F.O.slab;
  OctPass P = plan_pass(F, pass);
  if (pass == 2) {
    P.slab_z = S.np; P.chunk0 = S.chunk0; P.chunk_total = S.nb * S.nchunk; P.nchunk = S.nchunk; P.row_in = S.row_in.p; P.ng = S.ng;
    P.vec2 = 1;                              // (the planes in the exchange buffer are 16-byte aligned whatever the layout of the form's own vectors)
  } else {
    const bool first = pass == 1;
    P.slab_io = first ? 1 : 2; P.store_planes = S.own; P.scols = (int)S.scols; P.inv_scols = 1.0f / (float)S.scols; P.col_unit = S.nchunk * S.cw; P.rank = S.rank;
    P.dest_stride = (int64_t)((first ? S.max_own : S.max_nl) - 1) * S.scols; P.recv_off = S.recv_off;
  }
  return P;
}
// diagnostic (PORO_FDMO_STAMPS = file name): the third application of the process records the per-block time stamps of its three passes (OctPass::stamps) and
// writes them as lines "pass block t0 .. t5 hw_id xcc_id" (tools/fdmo_stamps.py)
struct PassStamps {
  bool on = false; DevBuf<unsigned long long> buf; int items[3] = {0, 0, 0};
  static const char *path() { static const char *p = std::getenv("PORO_FDMO_STAMPS"); return p; }
  PassStamps() { static int calls = 0; on = path() && ++calls == 3; }
  void attach(hipStream_t s, OctPass (&P)[3], const int (&n_items)[3]) {
    if (!on) return;
    buf.alloc((size_t)8 * (n_items[0] + n_items[1] + n_items[2])); buf.zero(s);
    for (int k = 0, at = 0; k < 3; at += n_items[k++]) { items[k] = n_items[k]; P[k].stamps = buf.p + 8 * (int64_t)at; }
  }
  void dump(hipStream_t s) {
    if (!on) return;
    PORO_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(buf.n); PORO_HIP(hipMemcpy(h.data(), buf.p, buf.n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE *f = std::fopen(path(), "w"); const unsigned long long *r = h.data();
    for (int pass = 0; f && pass < 3; ++pass) for (int b = 0; b < items[pass]; ++b, r += 8) std::fprintf(f, "%d %d %llu %llu %llu %llu %llu %llu %llu %llu\n", pass, b, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
    if (f) std::fclose(f);
  }
};
// sizes of a 3D form: half lines in the first `nsplit` directions (parity split, `no` parity parts), whole lines in the others; rows padded to even length where x is split.
// On slabs (slab_prologue first) the transformed z line is the global one, split in parities whenever x and y are.  coef != null (displacement system): g, z, t in the form's layout
void form_geometry(FdmOct &O, const int nn[3], const double (*coef)[3], int nsplit, int no, hipStream_t s) {
  const int zline = O.slab.on ? O.slab.ng : nn[2]; int hmax = nsplit ? (zline + 1) / 2 : zline;
  for (int d = 0; d < 3; ++d) {
    O.n[d] = nn[d]; O.h[d] = d < nsplit ? (nn[d] + 1) / 2 : nn[d];
    if (d < 2) hmax = std::max(hmax, O.h[d]);
    for (int c = 0; coef && c < 3; ++c) O.coef[c][d] = coef[c][d];
  }
  O.nt = O.nt_z = (hmax + 15) / 16; O.hxp = nsplit ? (O.h[0] + 1) & ~1 : O.h[0]; O.no = no;
  O.co_stride = (int64_t)O.hxp * O.h[1] * O.h[2]; O.n_oct = (coef ? 3 : 1) * no * O.co_stride;
  if (coef) { O.g.alloc(O.n_oct); O.z.alloc(O.n_oct); O.t.alloc(O.n_oct); O.g.zero(s); O.z.zero(s); O.t.zero(s); }
}
// slab forms: the ranks' layers -> global line length; this rank's planes must match its entry
void slab_prologue(FdmOct &O, const int nn[3], int rank, const std::vector<int> &node_layers, const char *who) {
  auto &S = O.slab; const int N = (int)node_layers.size();
  S.on = true; S.n_ranks = N; S.rank = rank;
  S.ng = 1; for (int q = 0; q < N; ++q) S.ng += node_layers[q];
  if (nn[2] != node_layers[rank] + 1) throw Error(std::string(who) + ": local planes do not match the layer table");
}

}  // namespace

// everything of the three passes of a displacement form that does not change from one application to the next: [fp64 / fp32 fragments][pass]
struct FdmoPlans { OctPass pass[2][3]; int n_items[3]; OctPassVM vm[3]; };

bool fdmo_usable(int dim, const int nn[3]) {
  if (dim != 3) return false;
  for (int d = 0; d < 3; ++d) if ((nn[d] + 1) / 2 > 16 * kFdmoMaxTiles || nn[d] < 2) return false;
  return true;
}

void fdmo_init(FdmOct &O, const int nn[3], const double coef[3][3], hipStream_t s) {
  form_geometry(O, nn, coef, 3, 8, s);
  // z doubles as the operator's nodal output h inside PCG (h and z are never live together, ctx.hip: solve_u_fdm): the octant array is the larger of the two (24 co >= n_u: 2 h >= n in every direction), checked here
  const int64_t n_u = (int64_t)3 * nn[0] * nn[1] * nn[2];
  if (n_u > O.n_oct) throw Error("fdmo_init: the octant array is smaller than the nodal vector");
  O.own_z = O.n[2];
  O.gz_n = 24 * pass2_chunks(O.hxp * O.h[1], O.nt);   // workgroups of pass 2: one g . z partial each (grows with the box - not bounded by kMaxPartials)
  O.gz_part.alloc(O.gz_n); O.gz_part.zero(s);
}
// Per-direction form (PORO_FDM_FORM_PER_DIRECTION; one rank, 3D): direction d is split in parities where D.split[d], else it keeps its whole line - no butterfly in the CG vector
// kernels, whole-length transforms.  Layout Q[c][part][kz][ky][kx] with 2^(split directions) parts per component; the row pitch is even whether or not x is split (16-byte
// block loads, paired accesses of the residual update; the pad entry is zero and stays zero).  Passes 1 / 3 and pass 2 have their own tile counts (D.nt_xy, D.nt_z), and
// every direction's fragments are packed for the pass that uses them
void fdmo_init_per_direction(FdmOct &O, const int nn[3], const double coef[3][3], const FdmFormDecision &D, hipStream_t s) {
  if (!D.usable) throw Error("fdmo_init_per_direction: a line of more than 128 entries");
  O.per_dir = true; O.split_mask = 0; O.no = 1;
  for (int d = 0; d < 3; ++d) {
    O.n[d] = nn[d]; O.h[d] = D.len[d];
    if (D.split[d]) { O.split_mask |= 1 << d; O.no *= 2; }
    for (int c = 0; c < 3; ++c) O.coef[c][d] = coef[c][d];
  }
  O.nt = D.nt_xy; O.nt_z = D.nt_z; O.hxp = (O.h[0] + 1) & ~1;
  O.co_stride = (int64_t)O.hxp * O.h[1] * O.h[2]; O.n_oct = (int64_t)3 * O.no * O.co_stride;
  // z doubles as the operator's nodal output h (fdmo_init): 2 h >= n in a split direction, h = n in a whole one, so the form's array holds the nodal vector - with equality,
  // up to the row pitch, where no direction is split
  if ((int64_t)3 * nn[0] * nn[1] * nn[2] > O.n_oct) throw Error("fdmo_init_per_direction: the form's array is smaller than the nodal vector");
  if (O.hxp > 16 * O.nt || O.h[1] > 16 * O.nt || O.h[2] > 16 * O.nt_z) throw Error("fdmo_init_per_direction: tile counts do not cover the lines");
  O.g.alloc(O.n_oct); O.z.alloc(O.n_oct); O.t.alloc(O.n_oct); O.g.zero(s); O.z.zero(s); O.t.zero(s);
  O.own_z = O.n[2];
  O.gz_n = 3 * O.no * pass2_chunks(O.hxp * O.h[1], O.nt_z);
  O.gz_part.alloc(O.gz_n); O.gz_part.zero(s);
}
// chunks, shares, plane tables and buffers of the slab form, after n / h / hxp / nt / co_stride are set: nb blocks per plane position set, np parity parts of a z line
static void slab_layout(FdmOct &O, int nb, int np, int rank, const std::vector<int> &node_layers, hipStream_t s) {
  auto &S = O.slab; const int N = (int)node_layers.size();
  S.nb = nb; S.np = np; S.hzg = np == 2 ? (S.ng + 1) / 2 : S.ng;
  const int64_t pl = (int64_t)O.hxp * O.h[1];
  // displacement system with 2, 4 or 5 tiles per half line: both parity parts of a z line in one workgroup (k_fdmo_zpass_both) - a chunk is then HALF a block wide
  S.zboth = np == 2 && (O.nt == 2 || O.nt == 4 || O.nt == 5) && !std::getenv("PORO_FDMO_SLAB_TWO_PARITY_WORKGROUPS");
  S.cw = S.zboth ? pass2_chunk(O.nt) / 2 : pass2_chunk(O.nt); S.nchunk = (int)((pl + S.cw - 1) / S.cw);
  const int chunk_total = nb * S.nchunk;
  S.cps = (chunk_total + N - 1) / N; S.chunk0 = rank * S.cps; S.my_chunks = std::max(0, std::min(S.cps, chunk_total - S.chunk0)); S.scols = (int64_t)S.cps * S.cw;
  std::vector<int> off(N), own(N), nl(N); int acc = 0; S.max_own = S.max_nl = S.rows_back = 0;
  for (int q = 0; q < N; ++q) { off[q] = acc; acc += node_layers[q]; own[q] = node_layers[q] + (q == N - 1 ? 1 : 0); nl[q] = node_layers[q] + 1; S.max_own = std::max(S.max_own, own[q]); S.max_nl = std::max(S.max_nl, nl[q]); S.rows_back += nl[q]; }
  S.own = own[rank]; S.nl = nl[rank];
  if ((int64_t)std::max(S.max_own, S.max_nl) * chunk_total * S.cw >= (int64_t)1 << 31 || (int64_t)S.rows_back * S.scols >= (int64_t)1 << 31 || (int64_t)chunk_total * S.cw >= (int64_t)1 << 24) throw Error("fdmo: a slab of more than 2^31 transform entries");
  // one buffer [send | recv]; what a rank keeps for itself is written straight into the receive half
  const int64_t blk = (int64_t)std::max(S.max_own, S.max_nl) * S.scols; S.recv_off = blk * N;
  std::vector<int64_t> rin(S.ng), rout(S.rows_back); std::vector<int32_t> rkz(S.rows_back);
  for (int q = 0; q < N; ++q) for (int k = 0; k < own[q]; ++k) rin[off[q] + k] = S.recv_off + ((int64_t)q * S.max_own + k) * S.scols;
  { int r = 0; for (int q = 0; q < N; ++q) for (int k = 0; k < nl[q]; ++k, ++r) { rout[r] = ((int64_t)q * S.max_nl + k) * S.scols + (q == rank ? S.recv_off : 0); rkz[r] = off[q] + k; } }
  S.row_in.upload(rin); S.row_out.upload(rout); S.row_kz.upload(rkz);
  { std::vector<int64_t> d2((size_t)2 * S.ng, -1);           // per global plane: where its rows go in the scattering all-to-all's buffer (one rank, or two for a shared plane)
    for (int r = 0; r < S.rows_back; ++r) { const int kz = rkz[r]; d2[2 * kz + (d2[2 * kz] >= 0 ? 1 : 0)] = rout[r]; }
    S.dst2.upload(d2); }
  S.buf.alloc((size_t)2 * blk * N); S.buf.zero(s);
  if (!S.zboth) { S.tz.alloc((size_t)np * S.cps * S.hzg * S.cw); S.tz.zero(s); }      // (the both-parity z pass goes from the gathered planes straight to the scattered ones)
}
void fdmo_init_slab(FdmOct &O, const int nn[3], const double coef[3][3], int rank, const std::vector<int> &node_layers, bool has_upper, hipStream_t s) {
  slab_prologue(O, nn, rank, node_layers, "fdmo_init_slab");
  form_geometry(O, nn, coef, 2, 4, s);
  O.own_z = has_upper ? nn[2] - 1 : nn[2];
  slab_layout(O, 12, 2, rank, node_layers, s);
}
// scalar Q1 system on a slab: nodal layout [local plane][y][x], whole-length lines everywhere (no parity split)
void fdmo_scalar_init_slab(FdmOct &O, const int nn[3], int rank, const std::vector<int> &node_layers, hipStream_t s) {
  slab_prologue(O, nn, rank, node_layers, "fdmo_scalar_init_slab");
  form_geometry(O, nn, nullptr, 0, 1, s);
  slab_layout(O, 1, 1, rank, node_layers, s);
}

// a whole direction of the per-direction form: every mode of the line (removed ones: zero columns of S, lam = inf), one matrix set in parity slot 0
static void fdmo_upload_dir_whole(FdmOct &O, int comp, int dir, const LineTables &T) {
  const int nt = dir == 2 ? O.nt_z : O.nt;
  std::vector<double> lp(16 * nt + 16, std::numeric_limits<double>::infinity());
  for (int m = 0; m < T.n; ++m) lp[m] = T.lam[m];
  O.h_lam[comp][dir][0] = lp; O.lam[comp][dir][0].upload(lp);
  O.fwd[comp][dir][0].upload(whole_line_fragments(T, nt, false)); O.bwd[comp][dir][0].upload(whole_line_fragments(T, nt, true));
}
void fdmo_upload_dir(FdmOct &O, int comp, int dir, const LineTables &T) {
  if (O.per_dir && T.n != O.n[dir]) throw Error("fdmo_upload_dir: line length mismatch");
  if (O.per_dir && !(O.split_mask & (1 << dir))) { fdmo_upload_dir_whole(O, comp, dir, T); return; }
  const int nn = T.n, h = (nn + 1) / 2, nt = dir == 2 ? O.nt_z : O.nt, padn = 16 * nt;      // (the tile count of the pass that uses the direction; one for all but the per-direction form)
  const std::vector<double> &S = T.S, &lam = T.lam;
  if (nn != (O.slab.on && dir == 2 ? O.slab.ng : O.n[dir])) throw Error("fdmo_upload_dir: line length mismatch");
  if (!T.parity) throw Error("fdmo_upload_dir: tables whose modes are not all even or odd");      // (the caller decides the form from T.parity before any upload)
  const std::vector<int> *const grp[2] = {&T.even, &T.odd};
  for (int p = 0; p < 2; ++p) {
    // forward F[m][k] = S[k][mode m] (rows = modes of the parity group, columns = lower-half nodes), backward B[k][m] = S[k][mode m]
    const std::vector<int> &g = *grp[p]; const int ng = (int)g.size();
    const std::vector<double> F = pack_fragments<double>(nt, 4 * nt, ng, h, [&](int r, int cc) { return S[(size_t)cc * nn + g[r]]; }), B = pack_fragments<double>(nt, 4 * nt, h, ng, [&](int r, int cc) { return S[(size_t)r * nn + g[cc]]; });
    std::vector<double> lp(padn + 16, std::numeric_limits<double>::infinity());
    for (int m = 0; m < ng; ++m) lp[m] = lam[g[m]];
    O.h_lam[comp][dir][p] = lp;
    O.fwd[comp][dir][p].upload(F); O.bwd[comp][dir][p].upload(B); O.lam[comp][dir][p].upload(lp);
    if (!O.slab.on && !O.per_dir) {   // fp32 mode of the octant form: both matrices rounded entry by entry from the same S, so the backward one is the exact transpose of the rounded forward one
      O.fwd32[comp][dir][p].upload(std::vector<float>(F.begin(), F.end())); O.bwd32[comp][dir][p].upload(std::vector<float>(B.begin(), B.end()));
    }
  }
}

void fdmo_upload_dir_classes(FdmOct &O, int comp, int dir, const ClassSplitTables &T) {
  if (!O.class_split || O.per_dir || O.slab.on || O.planar) throw Error("fdmo_upload_dir_classes: the class-split passes exist for the single-rank octant form only");
  if (!T.ok || T.n != O.n[dir]) throw Error("fdmo_upload_dir_classes: a line that is not class-split");      // (the caller decides from ClassSplitTables::ok before any upload)
  const int nt = O.nt, tiles = (nt + 1) / 2, ksteps = 2 * nt, h = O.h[dir]; const double inf = std::numeric_limits<double>::infinity();
  for (int p = 0; p < 2; ++p) {
    const ClassSplitGroup &G = T.grp[p];
    if (G.nv != (h + 1) / 2 || G.nm != h / 2 || G.nv > 8 * nt || G.slots > 8 * nt || G.slots > 64) throw Error("fdmo_upload_dir_classes: class sizes do not fit the pass kernel");
    for (int cls = 0; cls < 2; ++cls) { O.cfwd[comp][dir][p][cls].upload(class_fragments(G, cls, tiles, ksteps, false)); O.cbwd[comp][dir][p][cls].upload(class_fragments(G, cls, tiles, ksteps, true)); }
    std::vector<double> mix(4 * 64, 0.0), lam(2 * 64, inf);
    for (int s = 0; s < G.slots; ++s) { for (int e = 0; e < 4; ++e) mix[4 * s + e] = G.mix[4 * s + e]; lam[s] = G.lam_v[s]; lam[64 + s] = G.lam_m[s]; }
    O.cmix[comp][dir][p].upload(mix); O.clam[comp][dir][p].upload(lam); O.h_clam[comp][dir][p] = lam;
  }
}
bool fdmo_class_split_runs(const FdmOct &O, int precision) { return O.class_split && precision != PORO_FDM_FP32 && !O.per_dir && !O.slab.on && !O.planar; }

void fdmo_finalize(FdmOct &O) {
  const int hx = O.h[0], hy = O.h[1], hxp = O.hxp; const size_t pl = (size_t)hxp * hy;
  if (O.class_split) {      // the x / y share of the eigenvalue sums in the class-major mode order of the plane: index s of the vertex class, nv + s of the midpoint class
    const int nvx = (hx + 1) / 2, nvy = (hy + 1) / 2;
    std::vector<double> B((size_t)12 * pl, 1.0);
    for (int c = 0; c < 3; ++c) for (int q = 0; q < 4; ++q) for (int my = 0; my < hy; ++my) for (int mx = 0; mx < hx; ++mx) {
      const std::vector<double> &lx = O.h_clam[c][0][q & 1], &ly = O.h_clam[c][1][q >> 1];
      B[(size_t)(4 * c + q) * pl + (size_t)my * hxp + mx] = O.coef[c][0] * (mx < nvx ? lx[mx] : lx[64 + mx - nvx]) + O.coef[c][1] * (my < nvy ? ly[my] : ly[64 + my - nvy]);
    }
    O.bxy_vm.upload(B);
  }
  // planes per component: one per parity combination of x and y (per-direction form: of those of the two that are split, x in the lowest bit)
  const int sx = O.per_dir ? (O.split_mask & 1) : 1, sy = O.per_dir ? ((O.split_mask >> 1) & 1) : 1, cmul = 1 << (sx + sy);
  std::vector<double> B((size_t)3 * cmul * pl, 1.0);             // (row pads: any finite non-zero value, their data are zeros)
  for (int c = 0; c < 3; ++c) for (int q = 0; q < cmul; ++q) for (int my = 0; my < hy; ++my) for (int mx = 0; mx < hx; ++mx) {
    const int px = sx ? q & 1 : 0, py = sy ? (q >> sx) & 1 : 0;
    B[(size_t)(cmul * c + q) * pl + (size_t)my * hxp + mx] = O.coef[c][0] * O.h_lam[c][0][px][mx] + O.coef[c][1] * O.h_lam[c][1][py][my];
  }
  O.bxy.upload(B);
  auto plans = std::make_shared<FdmoPlans>();
  for (int f32 = 0; f32 < (O.slab.on || O.per_dir ? 1 : 2); ++f32) for (int k = 0; k < 3; ++k) {
    const Form F = disp_form(O, f32 != 0);
    plans->pass[f32][k] = O.slab.on ? plan_slab_pass(F, k + 1) : plan_pass(F, k + 1);
    plans->n_items[k] = F.blocks * plans->pass[f32][k].nblk;
  }
  if (O.class_split) for (int k = 0; k < 3; ++k) plans->vm[k] = plan_vm(O, plans->pass[0][k], k + 1);
  O.plans = plans;
}

void fdmo_apply(hipStream_t s, const FdmOct &O, const double *g_oct, double *z_oct, double *scratch, const PcgScalars *gate, hipEvent_t *ev, double *gz_part, int precision, const PcgStopTest &stop) {
  const bool f32 = precision == PORO_FDM_FP32;     // fp32 transforms: float fragments, `scratch` holds the intermediate array as floats (g_oct, z_oct stay fp64)
  if (f32 && (O.slab.on || O.planar || O.per_dir || !O.fwd32[0][0][0].p)) throw Error("fdmo_apply: fp32 transforms exist for the single-rank octant form only");
  OctPass P[3]; const int (&n_items)[3] = O.plans->n_items;
  for (int k = 0; k < 3; ++k) { P[k] = O.plans->pass[f32][k]; P[k].gate = gate; }
  if (gz_part && n_items[1] != O.gz_n) throw Error("fdmo_apply: the g.z partial buffer does not match the grid of pass 2");
  P[1].gz_part = gz_part;
  P[0].stop = stop;                                // (pass 1 is the first kernel of the call in either precision)
  if (stop.gg_part && stop.sc != gate) throw Error("fdmo_apply: a stopping test without the gate of its solve");
  PassStamps stamps; stamps.attach(s, P, n_items);
  // scratch == null (fp64 only): all three passes on z_oct itself, see "in place" at k_fdmo_pass.  The float intermediate of the fp32 mode needs its own array
  if (f32 && !scratch) throw Error("fdmo_apply: the fp32 transforms need the scratch array");
  double *const mid = scratch ? scratch : z_oct;
  const double *const in[3] = {g_oct, mid, mid}; double *const out[3] = {mid, mid, z_oct};      // (pass 2 works in place)
  if (fdmo_class_split_runs(O, precision)) {        // the same three launches with the class-split kernels (no stamps: the diagnostic belongs to k_fdmo_pass)
    for (int k = 0; k < 3; ++k) {
      OctPassVM V = O.plans->vm[k]; V.gate = gate; if (k == 1) V.gz_part = gz_part; if (k == 0) V.stop = stop;
      launch_vm_nt(s, O.nt, V, n_items[k], in[k], out[k], ev ? ev[2 * k] : nullptr, ev ? ev[2 * k + 1] : nullptr);
    }
    return;
  }
  for (int k = 0; k < 3; ++k) launch_pass_nt(s, k == 1 ? O.nt_z : O.nt, f32 ? PassVariant::OctantF32 : O.per_dir ? PassVariant::PerDirection : PassVariant::Octant, P[k], n_items[k], in[k], out[k], ev ? ev[2 * k] : nullptr, ev ? ev[2 * k + 1] : nullptr);
  stamps.dump(s);
}

// ---- slab form: the three sweeps as separate entry points (two all-to-alls sit between them, ctx_prec.hip) ----
void fdmo_slab_pass(hipStream_t s, const FdmOct &O, int pass, const double *in, double *out, const PcgScalars *gate, hipEvent_t e0, hipEvent_t e1) {
  const auto &S = O.slab;
  OctPass P = O.plans->pass[0][pass - 1]; P.gate = gate;
  if (pass != 2) launch_pass_nt(s, O.nt, PassVariant::SlabU, P, O.plans->n_items[pass - 1], in, out, e0, e1);
  else if (S.my_chunks <= 0) return;
  else if (!S.zboth) launch_pass_nt(s, O.nt, PassVariant::SlabU, P, 2 * S.my_chunks, in, out, e0, e1);
  else switch (O.nt) {       // both parity parts per workgroup: `in` and `out` are the exchange buffer (gathered planes in, scattered planes out)
    case 2: launch_zpass_both<2>(s, P, S.dst2.p, S.my_chunks, in, out, e0, e1); break;
    case 4: launch_zpass_both<4>(s, P, S.dst2.p, S.my_chunks, in, out, e0, e1); break;
    case 5: launch_zpass_both<5>(s, P, S.dst2.p, S.my_chunks, in, out, e0, e1); break;
    default: throw Error("fdmo: both-parity z pass needs 2, 4 or 5 tiles per half line");
  }
}
static int copy_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }
void fdmo_slab_scatter_pack(hipStream_t s, const FdmOct &O, const PcgScalars *gate) {
  const auto &S = O.slab; const SlabGeo G = geo_of(O);
  if (S.my_chunks > 0) hipLaunchKernelGGL(k_fdmo_slab_scatter_pack, copy_grid((int64_t)S.rows_back * S.my_chunks * S.cw), 256, 0, s, G, S.rows_back, S.row_out.p, S.row_kz.p, S.tz.p, S.buf.p, gate);
}
void fdmo_dot_owned(hipStream_t s, const FdmOct &O, const double *a, const double *b, double *partials, const PcgScalars *gate) {
  hipLaunchKernelGGL(k_fdmo_dot_owned, std::max(oct_grid(O.co_stride, O.nc), O.nc * O.no), kBlock, 0, s, dims_of(O), a, b, partials, gate);   // (at least one workgroup per block of the arrays)
}

// ---- the same three sweeps for a SCALAR Q1 system of the box (pressure Jacobian a M + kappa K, projection mass matrix): one "component", no parity octants, the
// vectors keep their nodal layout [z][y][x] (full-length lines, odd pitch: 8-byte block loads).  Replaces six single-direction launches of kernels_fdm.hip.
bool fdmo_scalar_usable(int dim, const int nn[3]) { if (dim != 3) return false; for (int d = 0; d < 3; ++d) if (nn[d] > 16 * kFdmoMaxTiles || nn[d] < 2) return false; return true; }
void fdmo_scalar_init(FdmOct &O, const int nn[3], hipStream_t s) {
  form_geometry(O, nn, nullptr, 0, 1, s);
  O.t.alloc(3 * O.n_oct); O.t.zero(s);      // (scratch for up to three right-hand sides at once)
}
void fdmo_scalar_upload_dir(FdmOct &O, int dir, const LineTables &T) {
  const int n = T.n; const std::vector<double> &S = T.S, &lam = T.lam;
  if (n != (O.slab.on && dir == 2 ? O.slab.ng : O.n[dir])) throw Error("fdmo_scalar_upload_dir: line length mismatch");
  std::vector<double> lp(16 * O.nt + 16, std::numeric_limits<double>::infinity());
  for (int m = 0; m < n; ++m) lp[m] = lam[m];
  O.h_lam[0][dir][0] = lp; O.lam[0][dir][0].upload(lp);
  O.fwd[0][dir][0].upload(pack_fragments<double>(O.nt, 4 * O.nt, n, n, [&](int r, int cc) { return S[(size_t)cc * n + r]; })); O.bwd[0][dir][0].upload(pack_fragments<double>(O.nt, 4 * O.nt, n, n, [&](int r, int cc) { return S[(size_t)r * n + cc]; }));
}
static const double *scalar_table(hipStream_t s, FdmOct &O, double a, double kappa);
// z = (a M + kappa K)^-1 g; the x / y share a + kappa (lam_x + lam_y) of the eigenvalue sums is tabulated per plane position, one table per (a, kappa)
int fdmo_scalar_apply(hipStream_t s, FdmOct &O, double a, double kappa, const double *g, double *z, const PcgScalars *gate) {
  const double *gs[1] = {g}; double *zs[1] = {z};
  return fdmo_scalar_apply_many(s, O, a, kappa, 1, gs, zs, gate);
}
// the strip form of a scalar pass (k_fdmo_strip): NT workgroups of NT waves per block (passes 1 / 3), 16-column chunks (pass 2)
template <int NT, int MODE> void launch_strip_one(hipStream_t s, int n_wg, const OctPass &P, const double *in, double *out) {
  constexpr unsigned lds = (unsigned)(PassGeom<NT>::PADN * (MODE == 1 ? 16 : PassGeom<NT>::LDMAX) * sizeof(double));
  if (lds > 64 * 1024) {
    static std::mutex mu; static std::set<int> done; int dev = 0; PORO_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (!done.count(dev)) { PORO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdmo_strip<NT, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); done.insert(dev); }
  }
  hipLaunchKernelGGL((k_fdmo_strip<NT, MODE>), dim3((unsigned)n_wg), dim3(64 * NT), lds, s, P, in, out);
}
template <int NT> void launch_strip(hipStream_t s, const OctPass &P, int n_items, const double *in, double *out) {
  if (P.mode == 0) launch_strip_one<NT, 0>(s, n_items * NT, P, in, out);
  else if (P.mode == 2) launch_strip_one<NT, 2>(s, n_items * NT, P, in, out);
  else launch_strip_one<NT, 1>(s, n_items, P, in, out);
}
void launch_strip_nt(hipStream_t s, int nt, const OctPass &P, int n_items, const double *in, double *out) {
  if (variant_of_flags(P) != PassVariant::General || P.slab_z || P.slab_io || P.row_in || P.no_shift || P.bxy_cmul || P.stop.gg_part || P.gz_part || P.stamps) throw Error("fdmo: the strip form serves the scalar passes of one rank only");
  switch (nt) {
    case 2: launch_strip<2>(s, P, n_items, in, out); break;
    case 3: launch_strip<3>(s, P, n_items, in, out); break;
    case 4: launch_strip<4>(s, P, n_items, in, out); break;
    case 5: launch_strip<5>(s, P, n_items, in, out); break;
    case 6: launch_strip<6>(s, P, n_items, in, out); break;
    case 7: launch_strip<7>(s, P, n_items, in, out); break;
    case 8: launch_strip<8>(s, P, n_items, in, out); break;
    default: throw Error("fdmo: lines of more than 128 entries");
  }
}
// the same for up to three right-hand sides in separate vectors: one set of three launches with 3 x the workgroups (the Q1 systems of config 4 fill less than a third of the chip)
// Strip form (k_fdmo_strip): a pass takes it when its block-per-workgroup launch would start fewer workgroups than O.strip_limit (kFdmoStripFill x the CUs of the device;
// 0 = the form is off).  Lines of one tile (nt = 1) have nothing to share out.  Returns the number of strip launches (the count-only timer family "fdm_q1_strip_launches")
int fdmo_scalar_apply_many(hipStream_t s, FdmOct &O, double a, double kappa, int nb, const double *const *g, double *const *z, const PcgScalars *gate) {
  if (nb < 1 || nb > 3) throw Error("fdmo_scalar_apply_many: 1..3 right-hand sides");
  const Form F = scalar_form(O, nb, kappa, scalar_table(s, O, a, kappa));
  const double *const in[3] = {g[0], O.t.p, O.t.p}; double *const out[3] = {O.t.p, O.t.p, z[0]};
  int strips = 0;
  for (int k = 0; k < 3; ++k) {
    OctPass P = plan_pass(F, k + 1);
    P.gate = gate;
    for (int c = 0; c < nb; ++c) { P.in_blk[c] = g[c]; P.out_blk[c] = z[c]; }
    P.use_in_off = k == 0; P.use_out_off = k == 2;           // pass 1 reads, pass 3 writes every right-hand side's own vector; in between they sit side by side in O.t
    const bool strip = O.nt >= 2 && !O.slab.on && (double)nb * P.nblk < O.strip_limit && g[0] != O.t.p && z[0] != O.t.p;
    if (!strip) { launch_pass_nt(s, O.nt, PassVariant::General, P, nb * P.nblk, in[k], out[k]); continue; }
    if (k == 1) { P.C = 16; P.blk_stride = 16; P.nblk = (P.pl + 15) / 16; }       // pass 2: 16-column chunks, the last one partial
    launch_strip_nt(s, O.nt, P, nb * P.nblk, in[k], out[k]);
    ++strips;
  }
  return strips;
}

static const double *scalar_table(hipStream_t s, FdmOct &O, double a, double kappa) {
  for (auto &T : O.scalar_tables) if (T.a == a && T.kappa == kappa) return T.t.p;
  const int hx = O.h[0], hy = O.h[1];
  if (O.scalar_tables.size() >= 8) { PORO_HIP(hipStreamSynchronize(s)); O.scalar_tables.pop_front(); }   // (a changing coefficient, e.g. a varying time step: drop the oldest)
  std::vector<double> Bt((size_t)hx * hy);
  // a removed mode (lam = inf: a line whose end node is prescribed) is marked inf outright - pass 2 then multiplies its coefficient by exactly 0 - instead of a + kappa inf,
  // which is NaN where kappa = 0
  const double inf = std::numeric_limits<double>::infinity();
  for (int my = 0; my < hy; ++my) for (int mx = 0; mx < hx; ++mx) {
    const double lx = O.h_lam[0][0][0][mx], ly = O.h_lam[0][1][0][my];
    Bt[(size_t)my * hx + mx] = (lx < 1e300 && ly < 1e300) ? a + kappa * (lx + ly) : inf;
  }
  O.scalar_tables.emplace_back(); auto &T = O.scalar_tables.back(); T.a = a; T.kappa = kappa; T.t.upload(Bt); return T.t.p;
}
void fdmo_scalar_slab_pass(hipStream_t s, FdmOct &O, int pass, double a, double kappa, const double *in, double *out) {
  const Form F = scalar_form(O, 1, kappa, scalar_table(s, O, a, kappa));
  const OctPass P = plan_slab_pass(F, pass);
  const int n_items = pass == 2 ? O.slab.my_chunks : P.nblk;
  if (n_items > 0) launch_pass_nt(s, O.nt, PassVariant::General, P, n_items, in, out);
}

#define PORO_OCT_LAUNCH(kernel, O, ...) do { if ((O).nc == 2) hipLaunchKernelGGL((kernel<2, false>), oct_grid((O).co_stride, 2), kBlock, 0, s, dims_of(O), __VA_ARGS__); \
                                              else if ((O).per_dir) hipLaunchKernelGGL((kernel<3, true>), oct_grid((O).co_stride, 3), kBlock, 0, s, dims_of(O), __VA_ARGS__); \
                                              else hipLaunchKernelGGL((kernel<3, false>), oct_grid((O).co_stride, 3), kBlock, 0, s, dims_of(O), __VA_ARGS__); } while (0)
// ---- planar form, host side: quadrant layout Q[c][2 py + px][ky][kx] (one plane), transforms as row-major h x h matrices F[mode][node] per (component, direction, parity) ----
bool fdmo_planar_usable(int dim, const int nn[3]) { return dim == 2 && nn[0] >= 2 && nn[1] >= 2 && nn[0] <= 4096 && nn[1] <= 4096; }
void fdmo_init_planar(FdmOct &O, const int nn[3], const double coef[3][3], hipStream_t s, bool split) {
  O.nc = 2; O.no = split ? 4 : 1; O.planar = true;
  for (int d = 0; d < 3; ++d) { O.n[d] = d < 2 ? nn[d] : 1; O.h[d] = d < 2 ? (split ? (nn[d] + 1) / 2 : nn[d]) : 1; for (int c = 0; c < 3; ++c) O.coef[c][d] = coef[c][d]; }
  O.nt = 0; O.hxp = (O.h[0] + 1) & ~1; O.own_z = 1;
  O.co_stride = (int64_t)O.hxp * O.h[1]; O.n_oct = 2 * O.no * O.co_stride;
  O.g.alloc(O.n_oct); O.z.alloc(O.n_oct); O.t.alloc(2 * O.n_oct);
  O.g.zero(s); O.z.zero(s); O.t.zero(s);
}
void fdmo_upload_dir_planar(FdmOct &O, int comp, int dir, const LineTables &T) {
  const int nn = T.n; const std::vector<double> &S = T.S, &lam = T.lam;
  if (nn != O.n[dir]) throw Error("fdmo_upload_dir_planar: line length mismatch");
  if (O.no == 1) {          // no parity split (different conditions at the two ends of a line): the full transform F[mode][node], modes that do not exist carry lam = inf
    std::vector<double> F((size_t)nn * nn, 0.0), lp((size_t)nn + 16, std::numeric_limits<double>::infinity());
    for (int m = 0; m < nn; ++m) { if (!(lam[m] < 1e300)) continue; for (int k = 0; k < nn; ++k) F[(size_t)m * nn + k] = S[(size_t)k * nn + m]; lp[m] = lam[m]; }
    O.h_lam[comp][dir][0] = lp; O.fwd[comp][dir][0].upload(F); O.lam[comp][dir][0].upload(lp);
    return;
  }
  const int h = (nn + 1) / 2;
  if (!T.parity) throw Error("fdmo_upload_dir_planar: tables whose modes are not all even or odd");
  const std::vector<int> *const grp[2] = {&T.even, &T.odd};
  for (int p = 0; p < 2; ++p) {
    std::vector<double> F((size_t)h * h, 0.0), lp((size_t)h + 16, std::numeric_limits<double>::infinity());
    const std::vector<int> &g = *grp[p]; const int ng = (int)g.size();
    for (int m = 0; m < ng; ++m) { for (int k = 0; k < h; ++k) F[(size_t)m * h + k] = S[(size_t)k * nn + g[m]]; lp[m] = lam[g[m]]; }
    O.h_lam[comp][dir][p] = lp; O.fwd[comp][dir][p].upload(F); O.lam[comp][dir][p].upload(lp);
  }
}
// z = blockdiag(A_cc)^-1 g in quadrant form: T = X Fx^T, U = (Fy T) / (cx lam_x + cy lam_y), V = Fy^T U, Z = V Fx  - four batched GEMMs over the 8 (component, quadrant) planes
void fdmo_apply_planar(hipStream_t s, const FdmOct &O, const double *g, double *z, const PcgScalars *gate, const PcgStopTest &stop) {
  const int hx = O.h[0], hy = O.h[1], hxp = O.hxp; const int64_t co = O.co_stride;
  double *t1 = O.t.p, *t2 = O.t.p + O.n_oct;
  const int no = O.no, nb = 2 * no;                 // blocks: (component, quadrant) - or the two components alone without the parity split
  if (stop.gg_part && stop.sc != gate) throw Error("fdmo_apply_planar: a stopping test without the gate of its solve");
  Gemm2D G{}; G.nb = nb; G.gate = gate; G.rsC = hxp; G.stop = stop;
  auto launch = [&](bool ak, bool bk) {
    const dim3 grid((unsigned)(((G.M + 63) / 64) * ((G.N + 63) / 64)), (unsigned)nb);
    if (ak && bk) hipLaunchKernelGGL((k_fdmo_gemm2d<true, true>), grid, 256, 0, s, G);
    else if (ak) hipLaunchKernelGGL((k_fdmo_gemm2d<true, false>), grid, 256, 0, s, G);
    else hipLaunchKernelGGL((k_fdmo_gemm2d<false, false>), grid, 256, 0, s, G);
  };
  // 1: T[ky][mx] = sum_kx X[ky][kx] Fx[mx][kx]
  G.M = hy; G.N = hx; G.K = hx; G.rsA = hxp; G.csA = 1; G.rsB = 1; G.csB = hx; G.scale = 0;
  for (int b = 0; b < nb; ++b) { const int c = b / no, q = b % no; G.A[b] = g + (int64_t)b * co; G.B[b] = O.fwd[c][0][q & 1].p; G.C[b] = t1 + (int64_t)b * co; }
  launch(true, true);
  G.stop = PcgStopTest{};                          // (the later GEMMs read the stored decision)
  // 2: U[my][mx] = sum_ky Fy[my][ky] T[ky][mx], divided by the eigenvalue sums
  G.M = hy; G.N = hx; G.K = hy; G.rsA = hy; G.csA = 1; G.rsB = hxp; G.csB = 1; G.scale = 1;
  for (int b = 0; b < nb; ++b) { const int c = b / no, q = b % no; G.A[b] = O.fwd[c][1][q >> 1].p; G.B[b] = t1 + (int64_t)b * co; G.C[b] = t2 + (int64_t)b * co;
                                G.lamM[b] = O.lam[c][1][q >> 1].p; G.lamN[b] = O.lam[c][0][q & 1].p; G.cM[b] = O.coef[c][1]; G.cN[b] = O.coef[c][0]; }
  launch(true, false);
  // 3: V[ky][mx] = sum_my Fy[my][ky] U[my][mx]
  G.rsA = 1; G.csA = hy; G.scale = 0;
  for (int b = 0; b < nb; ++b) { G.B[b] = t2 + (int64_t)b * co; G.C[b] = t1 + (int64_t)b * co; }
  launch(false, false);
  // 4: Z[ky][kx] = sum_mx V[ky][mx] Fx[mx][kx]
  G.M = hy; G.N = hx; G.K = hx; G.rsA = hxp; G.csA = 1; G.rsB = hx; G.csB = 1;
  for (int b = 0; b < nb; ++b) { const int c = b / no, q = b % no; G.A[b] = t1 + (int64_t)b * co; G.B[b] = O.fwd[c][0][q & 1].p; G.C[b] = z + (int64_t)b * co; }
  launch(true, false);
}

void fdmo_from_nodal(hipStream_t s, const FdmOct &O, const double *v, double *q) { PORO_OCT_LAUNCH(k_fdmo_from_nodal, O, v, (const uint8_t *)nullptr, q); }
void fdmo_to_nodal(hipStream_t s, const FdmOct &O, const double *r, double *v) { PORO_OCT_LAUNCH(k_fdmo_to_nodal, O, r, v); }
void fdmo_init_residual(hipStream_t s, const FdmOct &O, double *g, const double *Ax, const double *b, const uint8_t *inert) { PORO_OCT_LAUNCH(k_fdmo_init_residual, O, g, Ax, b, inert); }
void fdmo_first_direction(hipStream_t s, const FdmOct &O, double *d, const double *g, const double *z, double *partials) { PORO_OCT_LAUNCH(k_fdmo_first_direction, O, d, g, z, partials); }
void fdmo_update_g(hipStream_t s, const FdmOct &O, PcgScalars *sc, int parity, double *g, const double *h, const uint8_t *inert, const double *partials_dh, double *partials_out, const double *red) {
  static const bool single = std::getenv("PORO_FDMO_UPDATE_G_SINGLE") != nullptr;
  if (single) PORO_OCT_LAUNCH(k_fdmo_update_g, O, sc, parity, g, h, inert, partials_dh, partials_out, red);
  else PORO_OCT_LAUNCH(k_fdmo_update_g2, O, sc, parity, g, h, inert, partials_dh, partials_out, red);
}
template <int NC, bool XNT, bool PD> static void launch_update_d(hipStream_t s, const FdmOct &O, PcgScalars *sc, int parity, int it, double *x, double *d, const double *z, const double *partials_in, const double *red, bool gz_from_pass, int decided) {
  hipLaunchKernelGGL((k_fdmo_update_d<NC, XNT, PD>), oct_grid(O.co_stride, NC), kBlock, 0, s, dims_of(O), sc, parity, it, x, d, z, (int64_t)O.nc * O.n[0] * O.n[1] * O.n[2], partials_in, red,
                     gz_from_pass ? (const double *)O.gz_part.p : (const double *)nullptr, gz_from_pass ? O.gz_n : 0, decided);
}
void fdmo_update_d(hipStream_t s, const FdmOct &O, PcgScalars *sc, int parity, int it, double *x, double *d, const double *z, const double *partials_in, const double *red, bool gz_from_pass, bool stream_x, bool decided, bool gg_stored) {
  const int dec = decided ? (gg_stored && !red ? 2 : 1) : 0;
  if (O.nc == 2) launch_update_d<2, false, false>(s, O, sc, parity, it, x, d, z, partials_in, red, gz_from_pass, dec);       // (planar form)
  else if (O.per_dir && stream_x) launch_update_d<3, true, true>(s, O, sc, parity, it, x, d, z, partials_in, red, gz_from_pass, dec);
  else if (O.per_dir) launch_update_d<3, false, true>(s, O, sc, parity, it, x, d, z, partials_in, red, gz_from_pass, dec);
  else if (stream_x) launch_update_d<3, true, false>(s, O, sc, parity, it, x, d, z, partials_in, red, gz_from_pass, dec);
  else launch_update_d<3, false, false>(s, O, sc, parity, it, x, d, z, partials_in, red, gz_from_pass, dec);
}

}  // namespace poro
