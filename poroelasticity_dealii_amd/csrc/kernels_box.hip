// Uniform-box forms of the two cell loops that run every fixed-stress iteration besides the solves:
//   K-rhs-u : b_i = int alpha p_h div(phi_i)                      (PoroElasticDisplacementSolver.h:231-236 inside the loop :203-288)
//   K-proj  : r^c_i = int psi_i eps_c(u_h)                         (StrainProjector.h:150-195)
// On a box with constant Jacobian both are the SAME rectangular Kronecker operator and its transpose:
//   G_c = W^c_x (x) W^c_y (x) W^c_z,   W^c_d = D_d if d == c else N_d,
//   N_d[i][a] = int phi_i psi_a dx_d,  D_d[i][a] = int phi_i' psi_a dx_d      (1D Q_k x Q1, assembled from 2-column local blocks)
//   b_c = alpha G_c p + (lifting + Neumann),      r^(c,c) = G_c^T u_c,   r^(a,b) = (G_b^T u_a + G_a^T u_b) / 2.
// (The reference integrates these products with QGauss(k+1) / QGauss(2); both are exact for them, so the quadrature sums equal the
// 1D integrals up to rounding.)  One thread per OUTPUT node, gather form: no colouring, no atomics, no index arrays - the pressure
// vector (3 MB) and the 5^dim neighbourhood of u come through L1/L2, HBM sees each vector once.
// Each kernel has two forms with the same bits: the first as just described, the second (default; PORO_BOX_KERNELS=v1 selects the first) with contiguous
// stores and flagged lift / neu reads (K-rhs-u) and with the u neighbourhood staged in LDS (K-proj); see the comments at the kernels.
// The generic per-cell kernels (kernels_asm.hip) remain the path for unstructured meshes and check this one at set-up.
#include <cstdlib>
#include <cstring>
#include "common.hpp"

namespace poro {
namespace {

constexpr int kTB = 256;

// weights of direction d at u index i: nonzero p indices a0 .. a0+2 (entries may be zero / out of range -> weight 0)
struct W3 { int a0; double wN[3], wD[3]; };
template <int K> __device__ __forceinline__ W3 u_row_weights(const BoxCoupling &B, int d, int i) {
  constexpr int k = K; const int n = B.n[d], e = i / k, s = i - e * k;
  W3 w; w.wN[0] = w.wN[1] = w.wN[2] = 0; w.wD[0] = w.wD[1] = w.wD[2] = 0;
  if (s != 0) {                       // interior node of cell e
    w.a0 = e;
    w.wN[0] = B.N[1][0] * B.h[d]; w.wN[1] = B.N[1][1] * B.h[d]; w.wD[0] = B.D[1][0]; w.wD[1] = B.D[1][1];   // K = 2: the only interior node is s = 1
  } else {                            // vertex e: last node of cell e-1 and first node of cell e
    w.a0 = e - 1;
    if (e >= 1) { w.wN[0] += B.N[k][0] * B.h[d]; w.wN[1] += B.N[k][1] * B.h[d]; w.wD[0] += B.D[k][0]; w.wD[1] += B.D[k][1]; }
    if (e <= n - 1) { w.wN[1] += B.N[0][0] * B.h[d]; w.wN[2] += B.N[0][1] * B.h[d]; w.wD[1] += B.D[0][0]; w.wD[2] += B.D[0][1]; }
  }
  return w;
}

// acc[c] = (G_c p) at u node `node` (< the number of nodes): the first form's accumulation
template <int DIM, int K> __device__ __forceinline__ void box_rhs_u_node(const BoxCoupling &B, const double *__restrict__ p, int64_t node, double (&acc)[3]) {
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1;
  const int i0 = (int)(node % nu0), i1 = (int)((node / nu0) % nu1), i2 = (int)(node / ((int64_t)nu0 * nu1));
  const int np0 = B.n[0] + 1, np1 = B.n[1] + 1;
  const W3 w0 = u_row_weights<K>(B, 0, i0), w1 = u_row_weights<K>(B, 1, i1);
  W3 w2; w2.a0 = 0; w2.wN[0] = 1; w2.wN[1] = w2.wN[2] = 0; w2.wD[0] = w2.wD[1] = w2.wD[2] = 0;
  if constexpr (DIM == 3) w2 = u_row_weights<K>(B, 2, i2);
  acc[0] = acc[1] = acc[2] = 0;
#pragma unroll
  for (int c = 0; c < (DIM == 3 ? 3 : 1); ++c) {
    if (w2.wN[c] == 0.0 && w2.wD[c] == 0.0) continue;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (w1.wN[b] == 0.0 && w1.wD[b] == 0.0) continue;
      const double nn = w1.wN[b] * w2.wN[c], dn = w1.wD[b] * w2.wN[c], nd = w1.wN[b] * w2.wD[c];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (w0.wN[a] == 0.0 && w0.wD[a] == 0.0) continue;
        const double pv = p[(int64_t)(w0.a0 + a) + (int64_t)np0 * ((w1.a0 + b) + (int64_t)np1 * (w2.a0 + c))];
        acc[0] = fma(pv, w0.wD[a] * nn, acc[0]);
        acc[1] = fma(pv, w0.wN[a] * dn, acc[1]);
        if constexpr (DIM == 3) acc[2] = fma(pv, w0.wN[a] * nd, acc[2]);
      }
    }
  }
}
// The same sum, term by term, with all 3^DIM pressure values requested before the first of them is used (indices clamped into the box: a value that a zero weight skips
// is loaded and dropped).  In the form above every load sits behind the divergent skips of its term, so a thread waits for up to 27 loads one after the other
template <int DIM, int K, class I> __device__ __forceinline__ void box_rhs_u_node_preloaded(const BoxCoupling &B, const double *__restrict__ p, I node, double (&acc)[3]) {
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1;
  const int i0 = (int)(node % (I)nu0), i1 = (int)((node / (I)nu0) % (I)nu1), i2 = (int)(node / ((I)nu0 * (I)nu1));
  const int np0 = B.n[0] + 1, np1 = B.n[1] + 1, np2 = DIM == 3 ? B.n[2] + 1 : 1;
  const W3 w0 = u_row_weights<K>(B, 0, i0), w1 = u_row_weights<K>(B, 1, i1);
  W3 w2; w2.a0 = 0; w2.wN[0] = 1; w2.wN[1] = w2.wN[2] = 0; w2.wD[0] = w2.wD[1] = w2.wD[2] = 0;
  if constexpr (DIM == 3) w2 = u_row_weights<K>(B, 2, i2);
  constexpr int NC = DIM == 3 ? 3 : 1;
  double pv[NC][3][3];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int ia = min(max(w0.a0 + a, 0), np0 - 1), ib = min(max(w1.a0 + b, 0), np1 - 1), ic = min(max(w2.a0 + c, 0), np2 - 1);
        pv[c][b][a] = p[(int64_t)ia + (int64_t)np0 * (ib + (int64_t)np1 * ic)];
      }
  acc[0] = acc[1] = acc[2] = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (w2.wN[c] == 0.0 && w2.wD[c] == 0.0) continue;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (w1.wN[b] == 0.0 && w1.wD[b] == 0.0) continue;
      const double nn = w1.wN[b] * w2.wN[c], dn = w1.wD[b] * w2.wN[c], nd = w1.wN[b] * w2.wD[c];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (w0.wN[a] == 0.0 && w0.wD[a] == 0.0) continue;
        acc[0] = fma(pv[c][b][a], w0.wD[a] * nn, acc[0]);
        acc[1] = fma(pv[c][b][a], w0.wN[a] * dn, acc[1]);
        if constexpr (DIM == 3) acc[2] = fma(pv[c][b][a], w0.wN[a] * nd, acc[2]);
      }
    }
  }
}
__device__ __forceinline__ double box_rhs_u_finish(double alpha, double acc, double neu, double lift) { return (alpha * acc + neu) + lift; }      // same finish as k_rhs_u_finish

// First form (PORO_BOX_KERNELS=v1, and the reference of the tests): one thread per node stores its DIM dofs - 8-byte accesses at a stride of 8 DIM bytes in rhs, lift, neu and mask
template <int DIM, int K> __global__ void __launch_bounds__(kTB)
k_box_rhs_u(BoxCoupling B, double alpha, const double *__restrict__ p, const double *__restrict__ lift, const double *__restrict__ neu,
            const uint8_t *__restrict__ mask, double *__restrict__ rhs) {
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1, nu2 = DIM == 3 ? K * B.n[2] + 1 : 1;
  const int64_t node = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (node >= (int64_t)nu0 * nu1 * nu2) return;
  double acc[3];
  box_rhs_u_node<DIM, K>(B, p, node, acc);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    const int64_t dof = node * DIM + c;
    rhs[dof] = mask[dof] ? 0.0 : box_rhs_u_finish(alpha, acc[c], neu[dof], lift[dof]);
  }
}

// Second form: the same per-node sums (box_rhs_u_node_preloaded; I = 32 bits where the box has fewer than 2^31 nodes: 64-bit divisions are long instruction sequences), then the workgroup's kTB DIM dofs - one contiguous piece of every dof vector - go through LDS, so that a wave stores 64
// consecutive dofs and reads mask, lift and neu likewise.  lift and neu are zero except next to Dirichlet faces and on loaded faces: flags[t] (box_rhs_u_flags, built with
// the two arrays) tells whether the kRhsFlagDofs dofs [t kRhsFlagDofs, (t + 1) kRhsFlagDofs) - one 128-byte line of either array - hold any nonzero bits; where they do not,
// neither array is read and literal zeros enter the same finish (so the sign of a zero result is what it was).  flags == null: every line is read
constexpr int kRhsFlagDofs = 16;
static_assert(kTB % kRhsFlagDofs == 0, "a workgroup's dofs start on a flag boundary");
template <int DIM, int K> __global__ void __launch_bounds__(kTB)
k_box_rhs_u_v2(BoxCoupling B, double alpha, const double *__restrict__ p, const double *__restrict__ lift, const double *__restrict__ neu,
               const uint8_t *__restrict__ mask, const uint8_t *__restrict__ flags, double *__restrict__ rhs) {
  __shared__ double sacc[kTB * DIM];                   // (stores at a lane stride of DIM doubles.  DIM = 3: 6 banks, the 32 lanes of a ds_write_b64 group hit 32 different bank pairs; DIM = 2: two lanes per pair)
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1, nu2 = DIM == 3 ? K * B.n[2] + 1 : 1;
  const int64_t n_nodes = (int64_t)nu0 * nu1 * nu2, node = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (node < n_nodes) {
    double acc[3];
    if (n_nodes <= 0x7fffffff) box_rhs_u_node_preloaded<DIM, K, uint32_t>(B, p, (uint32_t)node, acc);
    else box_rhs_u_node_preloaded<DIM, K, int64_t>(B, p, node, acc);
#pragma unroll
    for (int c = 0; c < DIM; ++c) sacc[threadIdx.x * DIM + c] = acc[c];
  }
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * kTB * DIM, n_dofs = n_nodes * DIM;
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    const int l = r * kTB + threadIdx.x; const int64_t dof = first + l;
    if (dof >= n_dofs) break;                          // (dofs of nodes >= n_nodes: their sacc entries were not written)
    const bool any = !flags || flags[dof / kRhsFlagDofs];
    const double nv = any ? neu[dof] : 0.0, lv = any ? lift[dof] : 0.0;
    rhs[dof] = mask[dof] ? 0.0 : box_rhs_u_finish(alpha, sacc[l], nv, lv);
  }
}
// flags[t] = some entry of lift or neu among the dofs [16 t, 16 t + 16) is not +0.0 (bit pattern: -0.0 counts, the finish adds it)
__global__ void __launch_bounds__(kTB) k_box_rhs_u_flags(const double *__restrict__ lift, const double *__restrict__ neu, int64_t n, uint8_t *__restrict__ flags) {
  const int64_t dof = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const bool nz = dof < n && ((__double_as_longlong(lift[dof]) | __double_as_longlong(neu[dof])) != 0);
  const unsigned long long m = __ballot(nz);
  const int lane = threadIdx.x & 63;
  if (dof < n && lane % kRhsFlagDofs == 0) flags[dof / kRhsFlagDofs] = ((m >> lane) & 0xffffull) != 0;
}

// weights of direction d at p index a: u indices i0 .. i0+2k
struct W5 { int i0; double wN[5], wD[5]; };
template <int K> __device__ __forceinline__ W5 p_row_weights(const BoxCoupling &B, int d, int a) {
  constexpr int k = K; const int n = B.n[d];
  W5 w; w.i0 = k * (a - 1);
#pragma unroll
  for (int m = 0; m < 5; ++m) { w.wN[m] = 0; w.wD[m] = 0; }
#pragma unroll
  for (int s = 0; s <= k; ++s) {
    if (a >= 1) { w.wN[s] += B.N[s][1] * B.h[d]; w.wD[s] += B.D[s][1]; }                 // cell a-1, psi_1
    if (a <= n - 1) { w.wN[k + s] += B.N[s][0] * B.h[d]; w.wD[k + s] += B.D[s][0]; }     // cell a, psi_0
  }
  return w;
}

struct BoxProjOut { double *rhs[6]; int t1[6], t2[6]; int n; };

template <int DIM, int K> __global__ void __launch_bounds__(kTB)
k_box_proj_rhs(BoxCoupling B, const double *__restrict__ u, BoxProjOut out) {
  const int np0 = B.n[0] + 1, np1 = B.n[1] + 1, np2 = DIM == 3 ? B.n[2] + 1 : 1;
  const int64_t node = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (node >= (int64_t)np0 * np1 * np2) return;
  const int a0 = (int)(node % np0), a1 = (int)((node / np0) % np1), a2 = (int)(node / ((int64_t)np0 * np1));
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1;
  constexpr int span = 2 * K + 1;
  const W5 w0 = p_row_weights<K>(B, 0, a0), w1 = p_row_weights<K>(B, 1, a1);
  W5 w2; w2.i0 = 0; for (int m = 0; m < 5; ++m) { w2.wN[m] = 0; w2.wD[m] = 0; } w2.wN[0] = 1;
  if constexpr (DIM == 3) w2 = p_row_weights<K>(B, 2, a2);
  double G[DIM][DIM];                 // G[comp][dir] = int psi_node d u_comp / d x_dir
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int d = 0; d < DIM; ++d) G[c][d] = 0;
#pragma unroll
  for (int kz = 0; kz < (DIM == 3 ? span : 1); ++kz) {
    if (w2.wN[kz] == 0.0 && w2.wD[kz] == 0.0) continue;
#pragma unroll
    for (int jy = 0; jy < span; ++jy) {
      if (w1.wN[jy] == 0.0 && w1.wD[jy] == 0.0) continue;
      const double nn = w1.wN[jy] * w2.wN[kz], dn = w1.wD[jy] * w2.wN[kz], nd = w1.wN[jy] * w2.wD[kz];
      const int64_t rowbase = (int64_t)nu0 * ((w1.i0 + jy) + (int64_t)nu1 * (w2.i0 + kz));
#pragma unroll
      for (int ix = 0; ix < span; ++ix) {
        if (w0.wN[ix] == 0.0 && w0.wD[ix] == 0.0) continue;
        const double *uv = u + (rowbase + w0.i0 + ix) * DIM;
        const double gx = w0.wD[ix] * nn, gy = w0.wN[ix] * dn, gz = w0.wN[ix] * nd;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const double uc = uv[c];
          G[c][0] = fma(uc, gx, G[c][0]); G[c][1] = fma(uc, gy, G[c][1]);
          if constexpr (DIM == 3) G[c][2] = fma(uc, gz, G[c][2]);
        }
      }
    }
  }
  auto sel = [&](int c, int d) {
    double r = 0;
#pragma unroll
    for (int cc = 0; cc < DIM; ++cc)
#pragma unroll
      for (int dd = 0; dd < DIM; ++dd) if (cc == c && dd == d) r = G[cc][dd];
    return r;
  };
  for (int e = 0; e < out.n; ++e) {
    const int t1 = out.t1[e], t2 = out.t2[e];
    out.rhs[e][node] = t1 == t2 ? sel(t1, t1) : (sel(t1, t2) + sel(t2, t1)) / 2;   // StrainProjector.h:177-181 / ConstitutiveModel.h:27-42
  }
}

// Second form.  The first one gathers (2 K + 1)^DIM u nodes x DIM components per thread straight from global memory, neighbouring lanes 8 K DIM bytes apart: 375 scattered
// 8-byte loads per thread at Q2 in 3D.  Here a workgroup owns kPT x kPT pressure nodes of ONE z plane and walks the 2 K + 1 u planes that plane touches: each u plane's
// (K kPT + K + 1)^2 nodes are staged in LDS with coalesced loads (whole rows of the tile are contiguous in u), and every thread runs the first form's accumulation from LDS - same kz, jy, ix order, same products, same skips, so the same bits.  A plane whose z weights
// are both zero (outside the box) is skipped by the whole workgroup, as every thread of it skips it in the first form.
// LDS layout per component: [tile row][column % K][column / K], pitch PH: thread (tx, ty) reads column K tx + ix of row K ty + jy, so the 16 lanes of a tile row read 16
// consecutive doubles and the next tile row lies K K PH doubles further - PH is chosen such that this is 16 (mod 32): the 32 lanes that a ds_read_b64 serves together
// hit 32 different bank pairs.  Out-of-box entries of a tile are staged as zeros and only ever meet skipped (zero-weight) terms.
constexpr int kPT = 16;
static_assert(kPT * kPT == kTB, "one thread per pressure node of the tile");
template <int DIM, int K> struct ProjTile {
  static constexpr int U = K * kPT + K + 1;                 // u nodes per direction under the tile: K (a - 1) .. K (a + kPT - 1 - 1) + 2 K
  static constexpr int NH = (U - 1) / K + 1;                // entries per (row, phase)
  static constexpr int PH = K == 1 ? 48 : 20;               // K K PH = 16 (mod 32), PH >= NH
  static constexpr int PLANE = U * K * PH;                  // doubles per component
  static_assert(K == 1 || K == 2, "Q1 or Q2 displacements");
  static_assert(PH >= NH && (K * K * PH) % 32 == 16, "LDS pitch");
};
template <int DIM, int K> __global__ void __launch_bounds__(kTB)
k_box_proj_rhs_v2(BoxCoupling B, const double *__restrict__ u, BoxProjOut out) {
  typedef ProjTile<DIM, K> T;
  __shared__ double su[DIM * T::PLANE];
  const int np0 = B.n[0] + 1, np1 = B.n[1] + 1;
  const int nu0 = K * B.n[0] + 1, nu1 = K * B.n[1] + 1, nu2 = DIM == 3 ? K * B.n[2] + 1 : 1;
  const int tid = threadIdx.x, tx = tid % kPT, ty = tid / kPT;
  const int a0 = blockIdx.x * kPT + tx, a1 = blockIdx.y * kPT + ty, a2 = DIM == 3 ? blockIdx.z : 0;
  const bool inside = a0 < np0 && a1 < np1;
  constexpr int span = 2 * K + 1;
  // (threads past the box edge take the last node's weights: they stage and wait at the barriers with the others, accumulate nothing and store nothing)
  const W5 w0 = p_row_weights<K>(B, 0, min(a0, np0 - 1)), w1 = p_row_weights<K>(B, 1, min(a1, np1 - 1));
  W5 w2; w2.i0 = 0; for (int m = 0; m < 5; ++m) { w2.wN[m] = 0; w2.wD[m] = 0; } w2.wN[0] = 1;
  if constexpr (DIM == 3) w2 = p_row_weights<K>(B, 2, a2);
  // The z weights are the workgroup's and the y weights a tile row's: kept in LDS and read back by a run-time index, so that the plane loop and the row loop below stay
  // loops.  (Unrolled like the first form's, the 25 (kz, jy) bodies with their LDS loads hoisted cost 231 registers at Q2 in 3D: two waves per SIMD.)
  __shared__ double sw2N[5], sw2D[5], sw1N[kPT][5], sw1D[kPT][5];
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < 5; ++m) { sw2N[m] = w2.wN[m]; sw2D[m] = w2.wD[m]; }
  }
  if (tx == 0) {
#pragma unroll
    for (int m = 0; m < 5; ++m) { sw1N[ty][m] = w1.wN[m]; sw1D[ty][m] = w1.wD[m]; }
  }
  const int gz0 = w2.i0;
  __syncthreads();
  const int ux0 = K * ((int)blockIdx.x * kPT - 1), uy0 = K * ((int)blockIdx.y * kPT - 1);       // first u column / row under the tile (may be -K)
  // staging: half a workgroup per tile row (a row's U DIM doubles are contiguous in u), kRowsPer rows at a time - all their loads are issued before the first LDS store.
  // Every address is one base plus a compile-time multiple of the row pitch
  constexpr int kHalf = kTB / 2, kRowsPer = 9, kRowSteps = (T::U + 1) / 2;
  static_assert(T::U * DIM <= kHalf, "a tile row fits half a workgroup");
  const int srem = tid % kHalf, scol = srem / DIM, sc = srem - scol * DIM, srow0 = tid / kHalf;
  const bool scol_ok = srem < T::U * DIM && ux0 + scol >= 0 && ux0 + scol < nu0;
  const int slds = sc * T::PLANE + (srow0 * K + scol % K) * T::PH + scol / K;
  auto stage_plane = [&](int kz) {          // u plane gz0 + kz under the tile -> LDS
    const int gz = gz0 + kz;
    const bool plane_ok = scol_ok && gz >= 0 && gz < nu2;      // (a live plane lies in the box)
    const double *up = u + ((int64_t)nu0 * (uy0 + srow0 + (int64_t)nu1 * gz) + ux0 + scol) * DIM + sc;
#pragma unroll
    for (int q0 = 0; q0 < kRowSteps; q0 += kRowsPer) {
      double stage[kRowsPer];
#pragma unroll
      for (int q = q0; q < q0 + kRowsPer && q < kRowSteps; ++q) {
        const int row = 2 * q + srow0, gy = uy0 + row;
        const bool ok = plane_ok && row < T::U && gy >= 0 && gy < nu1;
        stage[q - q0] = ok ? up[(int64_t)(2 * q) * nu0 * DIM] : 0.0;
      }
#pragma unroll
      for (int q = q0; q < q0 + kRowsPer && q < kRowSteps; ++q)
        if (srem < T::U * DIM && 2 * q + srow0 < T::U) su[slds + 2 * q * K * T::PH] = stage[q - q0];
    }
  };
  auto live = [&](int kz) { return !(sw2N[kz] == 0.0 && sw2D[kz] == 0.0); };      // (workgroup-uniform: a2 is)
  double G[DIM][DIM];                 // G[comp][dir] = int psi_node d u_comp / d x_dir
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int d = 0; d < DIM; ++d) G[c][d] = 0;
#pragma unroll 1
  for (int kz = 0; kz < (DIM == 3 ? span : 1); ++kz) {
    if (!live(kz)) continue;
    const double w2N = sw2N[kz], w2D = sw2D[kz];
    __syncthreads();                  // the previous plane has been read by everybody
    stage_plane(kz);
    __syncthreads();
    if (!inside) continue;
#pragma unroll 1
    for (int jy = 0; jy < span; ++jy) {
      const double w1N = sw1N[ty][jy], w1D = sw1D[ty][jy];
      if (w1N == 0.0 && w1D == 0.0) continue;
      const double nn = w1N * w2N, dn = w1D * w2N, nd = w1N * w2D;
      const int rowbase = ((K * ty + jy) * K) * T::PH + tx;
#pragma unroll
      for (int ix = 0; ix < span; ++ix) {
        if (w0.wN[ix] == 0.0 && w0.wD[ix] == 0.0) continue;
        const double *uv = su + rowbase + (ix % K) * T::PH + ix / K;
        const double gx = w0.wD[ix] * nn, gy = w0.wN[ix] * dn, gz = w0.wN[ix] * nd;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const double uc = uv[c * T::PLANE];
          G[c][0] = fma(uc, gx, G[c][0]); G[c][1] = fma(uc, gy, G[c][1]);
          if constexpr (DIM == 3) G[c][2] = fma(uc, gz, G[c][2]);
        }
      }
    }
  }
  if (!inside) return;
  const int64_t node = a0 + (int64_t)np0 * (a1 + (int64_t)np1 * a2);
  auto sel = [&](int c, int d) {
    double r = 0;
#pragma unroll
    for (int cc = 0; cc < DIM; ++cc)
#pragma unroll
      for (int dd = 0; dd < DIM; ++dd) if (cc == c && dd == d) r = G[cc][dd];
    return r;
  };
  for (int e = 0; e < out.n; ++e) {
    const int t1 = out.t1[e], t2 = out.t2[e];
    out.rhs[e][node] = t1 == t2 ? sel(t1, t1) : (sel(t1, t2) + sel(t2, t1)) / 2;
  }
}

// ---- K-asm-u on a uniform box: every cell matrix is the same Ke, so each CSR entry is written ONCE by its owner (no colouring, no
// read-modify-write): A(r, c) = sum over the <= 2^dim cells that contain both nodes of Ke[local(r)][local(c)], Dirichlet rows / columns
// eliminated as in distribute_local_to_global (sum of |K_ii| on the constrained diagonal).  L lanes per CSR row as in k_spmv.
// x / d for 0 <= x < 2^31 through the reciprocal (one correction step): the kernel decomposes a node index per CSR entry
__device__ __forceinline__ int div_by(int x, int d, double inv) { int q = (int)((double)x * inv); const int r = x - q * d; if (r < 0) --q; else if (r >= d) ++q; return q; }
template <int DIM, int K, int L> __global__ void __launch_bounds__(256)
k_box_asm_u(int n0, int n1, int n2, const double *__restrict__ Ke, int64_t n_rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
            const uint8_t *__restrict__ mask, double *__restrict__ val) {
  constexpr int N1 = K + 1, NS = DIM == 2 ? N1 * N1 : N1 * N1 * N1, DPC = NS * DIM;
  const int lane = threadIdx.x % L;
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  if (row >= n_rows) return;
  const int nc[3] = {n0, n1, n2};
  const int nx = K * n0 + 1, ny = K * n1 + 1;
  const double inx = 1.0 / nx, iny = 1.0 / ny;
  const int node_r = (int)(row / DIM), cr = (int)(row - (int64_t)node_r * DIM);
  const int qr = div_by(node_r, nx, inx), zr = DIM == 3 ? div_by(qr, ny, iny) : 0;
  const int ir[3] = {node_r - qr * nx, qr - zr * ny, zr};
  const bool mrow = mask[row] != 0;
  for (int64_t e = rp[row] + lane; e < rp[row + 1]; e += L) {
    const int32_t c = col[e];
    const int node_c = c / DIM, cc = c - node_c * DIM;
    const int qc = div_by(node_c, nx, inx), zc = DIM == 3 ? div_by(qc, ny, iny) : 0;
    const int ic[3] = {node_c - qc * nx, qc - zc * ny, zc};
    int c0[3], cnt[3];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {                            // cells of direction d that contain both indices: K c <= i, j <= K c + K
      const int hi = ir[d] > ic[d] ? ir[d] : ic[d], lo = ir[d] < ic[d] ? ir[d] : ic[d];
      int cmin = (hi - K + K - 1) / K; if (hi - K < 0) cmin = 0;
      int cmax = lo / K; if (cmax > nc[d] - 1) cmax = nc[d] - 1;
      c0[d] = cmin; cnt[d] = cmax - cmin + 1;
    }
    double v = 0.0;
    const bool diag = c == (int32_t)row;
    if (!(mrow && !diag) && !(mask[c] && !mrow)) {
      for (int kz = 0; kz < (DIM == 3 ? cnt[2] : 1); ++kz)
        for (int ky = 0; ky < cnt[1]; ++ky)
          for (int kx = 0; kx < cnt[0]; ++kx) {
            const int cx = c0[0] + kx, cy = c0[1] + ky, cz = DIM == 3 ? c0[2] + kz : 0;
            const int li = (DIM == 3 ? (ir[2] - K * cz) * N1 * N1 : 0) + (ir[1] - K * cy) * N1 + (ir[0] - K * cx);
            const int lj = (DIM == 3 ? (ic[2] - K * cz) * N1 * N1 : 0) + (ic[1] - K * cy) * N1 + (ic[0] - K * cx);
            const double k = Ke[(size_t)(li * DIM + cr) * DPC + lj * DIM + cc];
            v += mrow ? fabs(k) : k;
          }
    }
    val[e] = v;
  }
}

}  // namespace

template <int DIM, int K> static void launch_box_asm(hipStream_t s, const BoxDev &box, const double *Ke, const CsrDev &A, const uint8_t *mask, double *val) {
  const int64_t grid = (A.n * 64 + 255) / 256;
  hipLaunchKernelGGL((k_box_asm_u<DIM, K, 64>), (unsigned)grid, 256, 0, s, box.n[0], box.n[1], DIM == 3 ? box.n[2] : 1, Ke, A.n, A.rp.p, A.col.p, mask, val);
}
void box_asm_u_matrix(hipStream_t s, int dim, int k_u, const BoxDev &box, const double *Ke, const CsrDev &A, const uint8_t *mask, double *val) {
  if (dim == 2 && k_u == 1) launch_box_asm<2, 1>(s, box, Ke, A, mask, val);
  else if (dim == 2) launch_box_asm<2, 2>(s, box, Ke, A, mask, val);
  else if (k_u == 1) launch_box_asm<3, 1>(s, box, Ke, A, mask, val);
  else launch_box_asm<3, 2>(s, box, Ke, A, mask, val);
}

// 1D local blocks on the unit interval: N[s][t] = int phi_s psi_t, D[s][t] = int phi_s' psi_t (Lagrange Q_k on equidistant nodes, Q1)
BoxCoupling box_coupling(int dim, int k_u, const BoxDev &box) {
  if (k_u < 1 || k_u > 2) throw Error("box assembly: displacement degree must be 1 or 2");
  BoxCoupling B{}; B.k = k_u;
  for (int d = 0; d < 3; ++d) { B.n[d] = d < dim ? box.n[d] : 1; B.h[d] = d < dim ? box.h[d] : 1.0; }
  static const double gx[3] = {0.5 - 0.3872983346207417, 0.5, 0.5 + 0.3872983346207417}, gw[3] = {5.0 / 18, 8.0 / 18, 5.0 / 18};   // exact to degree 5
  const int ns = k_u + 1;
  for (int s = 0; s < ns; ++s)
    for (int t = 0; t < 2; ++t) {
      double vn = 0, vd = 0;
      for (int q = 0; q < 3; ++q) {
        const double x = gx[q];
        double phi = 1, dphi = 0;                        // Lagrange basis s on nodes j / k
        for (int j = 0; j < ns; ++j) if (j != s) phi *= (x - (double)j / k_u) / ((double)(s - j) / k_u);
        for (int m = 0; m < ns; ++m) if (m != s) { double term = 1.0 / ((double)(s - m) / k_u); for (int j = 0; j < ns; ++j) if (j != s && j != m) term *= (x - (double)j / k_u) / ((double)(s - j) / k_u); dphi += term; }
        const double psi = t ? x : 1 - x;
        vn += gw[q] * phi * psi; vd += gw[q] * dphi * psi;
      }
      B.N[s][t] = vn; B.D[s][t] = vd;
    }
  return B;
}

// PORO_BOX_KERNELS=v1 (A/B hook, read per call): the first forms of k_box_rhs_u and k_box_proj_rhs
static bool box_kernels_v1() { const char *e = std::getenv("PORO_BOX_KERNELS"); return e && std::strcmp(e, "v1") == 0; }

int64_t box_rhs_u_flag_count(int64_t n_u) { return (n_u + kRhsFlagDofs - 1) / kRhsFlagDofs; }
void box_rhs_u_flags(hipStream_t s, const double *lift, const double *neu, int64_t n_u, uint8_t *flags) {
  if (n_u > 0) hipLaunchKernelGGL(k_box_rhs_u_flags, (unsigned)((n_u + kTB - 1) / kTB), kTB, 0, s, lift, neu, n_u, flags);
}
void box_rhs_u(hipStream_t s, int dim, const BoxCoupling &B, double alpha, const double *p, const double *lift, const double *neu, const uint8_t *mask, double *rhs, const uint8_t *flags) {
  int64_t nn = 1; for (int d = 0; d < dim; ++d) nn *= (int64_t)B.k * B.n[d] + 1;
  const unsigned grid = (unsigned)((nn + kTB - 1) / kTB);
  if (!box_kernels_v1()) {
    if (dim == 2 && B.k == 1) hipLaunchKernelGGL((k_box_rhs_u_v2<2, 1>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, flags, rhs);
    else if (dim == 2) hipLaunchKernelGGL((k_box_rhs_u_v2<2, 2>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, flags, rhs);
    else if (B.k == 1) hipLaunchKernelGGL((k_box_rhs_u_v2<3, 1>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, flags, rhs);
    else hipLaunchKernelGGL((k_box_rhs_u_v2<3, 2>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, flags, rhs);
    return;
  }
  if (dim == 2 && B.k == 1) hipLaunchKernelGGL((k_box_rhs_u<2, 1>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, rhs);
  else if (dim == 2) hipLaunchKernelGGL((k_box_rhs_u<2, 2>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, rhs);
  else if (B.k == 1) hipLaunchKernelGGL((k_box_rhs_u<3, 1>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, rhs);
  else hipLaunchKernelGGL((k_box_rhs_u<3, 2>), grid, kTB, 0, s, B, alpha, p, lift, neu, mask, rhs);
}

void box_proj_rhs(hipStream_t s, int dim, const BoxCoupling &B, const double *u, int n_comp, const int32_t *tensor_components, double *const *rhs) {
  int64_t nn = 1; for (int d = 0; d < dim; ++d) nn *= (int64_t)B.n[d] + 1;
  BoxProjOut out{}; out.n = n_comp;
  for (int e = 0; e < n_comp; ++e) { out.rhs[e] = rhs[e]; out.t1[e] = tensor_components[e] / dim; out.t2[e] = tensor_components[e] % dim; }
  if (!box_kernels_v1()) {
    const dim3 tiles((unsigned)((B.n[0] + 1 + kPT - 1) / kPT), (unsigned)((B.n[1] + 1 + kPT - 1) / kPT), dim == 3 ? (unsigned)(B.n[2] + 1) : 1u);
    if (tiles.z > 65535u) throw Error("box_proj_rhs: more than 65535 pressure planes");
    if (dim == 2 && B.k == 1) hipLaunchKernelGGL((k_box_proj_rhs_v2<2, 1>), tiles, kTB, 0, s, B, u, out);
    else if (dim == 2) hipLaunchKernelGGL((k_box_proj_rhs_v2<2, 2>), tiles, kTB, 0, s, B, u, out);
    else if (B.k == 1) hipLaunchKernelGGL((k_box_proj_rhs_v2<3, 1>), tiles, kTB, 0, s, B, u, out);
    else hipLaunchKernelGGL((k_box_proj_rhs_v2<3, 2>), tiles, kTB, 0, s, B, u, out);
    return;
  }
  const unsigned grid = (unsigned)((nn + kTB - 1) / kTB);
  if (dim == 2 && B.k == 1) hipLaunchKernelGGL((k_box_proj_rhs<2, 1>), grid, kTB, 0, s, B, u, out);
  else if (dim == 2) hipLaunchKernelGGL((k_box_proj_rhs<2, 2>), grid, kTB, 0, s, B, u, out);
  else if (B.k == 1) hipLaunchKernelGGL((k_box_proj_rhs<3, 1>), grid, kTB, 0, s, B, u, out);
  else hipLaunchKernelGGL((k_box_proj_rhs<3, 2>), grid, kTB, 0, s, B, u, out);
}

}  // namespace poro
