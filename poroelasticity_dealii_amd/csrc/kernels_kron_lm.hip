// K-apply-u, sum-factorised form on a uniform 3D box whose Lame lambda and shear modulus G are constant within every cell layer of z (gfx950, wave64).
//
// With lambda(z), G(z) the operator is still a sum of Kronecker products of 1D matrices; only the z factor carries the weight (Mz^w = sum_l w_l M_l, K and C alike):
//   A_aa = sum_d F_x (x) F_y (x) F_z^w,  w = lambda + 2G (d == a) | G,  F_d = K, the others M
//   A_ab = C_a (x) C_b^T [lambda] + C_a^T (x) C_b [G]   (a != b),  M in the third direction
// (C[m][n] = int phi_m' phi_n as in kernels_kron.hip; checked against a per-cell quadrature assembly in tests/test_moduli_structured_cpu.py).  The construction is that
// of kernels_kron.hip - a 1024-node tile column marching along z, a register window of the planes around the current one, y through LDS, x by DPP shifts, out-of-range
// buffer offsets in place of branches, the Dirichlet-column mask applied as a plane enters the window, z-major tile numbering over the XCDs, z-chunks, no atomics - with
// these differences:
//   z: the weights enter the z-stage sums.  A vertex plane between the layers lo and hi adds the two one-sided halves of every band row (M, K, C with its diagonal,
//      C^T), each times that side's weight; a mid plane (Q2) uses its layer's weight.  The weights come from a per-plane table (moduli_planes.hpp: lambda_lo, G_lo,
//      lambda_hi, G_hi; zeros where the box ends, which stand in for the mL / mR of the constant kernel).  The table index is wave-uniform: ordinary loads that the
//      compiler makes scalar.  The diagonal of C_z^w, 3 (w_lo - w_hi) / 6 for Q2, is non-zero on every interface plane, so it is part of the z-stage fields and the
//      constant kernel's second LDS round for the first / last plane does not exist here.
//   fields: 14 per plane instead of 9, with u_c the components of the plane's window and T = C^T
//        0 Mz^l u_x   1 Mz^G u_x   2 Mz^l u_y   3 Mz^G u_y   4 Mz^G u_z                       (Mz^l u_z has no consumer: A_zz holds Mz^G only)
//        5 Kz^G u_x   6 Kz^G u_y   7 Kz^(l+2G) u_z
//        8 Tz^l u_z - Cz^G u_z     9 Tz^l u_z + Cz^G u_z                                       (coupling of u_z into y_x, y_y)
//       10 Tz^G u_x - Cz^l u_x    11 Tz^G u_x + Cz^l u_x    12, 13 the same of u_y             (coupling of u_x, u_y into y_z)
//      lambda and G no longer multiply after the y-stage: the scales hold the sM, sK, sC factors of the integer 1D matrices alone.
//   LDS: one buffer of 14 x 1024 doubles (112 KiB of the 160 KiB of a CU; two do not fit) and two barriers per plane.  The z-stage of a plane is computed in registers
//      BEFORE the first barrier (the one that waits for the readers of the previous plane), so only the LDS writes sit between the two.
// Results are bitwise reproducible; the Dirichlet rows hold the unconstrained row sums as in kernels_kron.hip (kron_fix_constrained finishes them).
#include "common.hpp"
#include <hip/hip_ext.h>
#include <type_traits>

namespace poro {
namespace {

constexpr int NF = 14;              // z-stage fields of a plane
constexpr int kTileNodes = 1024;
constexpr int kPad = 64;            // doubles in front of and behind the plane buffer: the rows -1 and TYR that the Q1 32-lane tile's edge rows read (never used)

struct LmScales { double xk, ky, kz, cz, oz, mx; };   // sKx sMy sMz | sMx sKy sMz | sMx sMy sKz | sC sC sMz | sC sMy sC | sMx sC sC
struct LmArgs {
  int nn[3]; int n64, nty64, has32, nty32, x0_32, nzc, zunit, zq, zr, nA, nblocks, cols;   // the tiling of kernels_kron.hip (z-major numbering)
  LmScales k;
  const uint8_t *nodemask; int constrained, mask_anywhere;
  double *dot_partials;     // optional: per-workgroup partial of x.y over the free rows
  const PcgScalars *pcg;    // optional: no-op once the solve has finished
};

__device__ inline int64_t xcd_remap(int64_t bid, int64_t n) {
  const int64_t q = n / 8, r = n % 8, xcd = bid % 8, idx = bid / 8;
  return xcd * q + (xcd < r ? xcd : r) + idx;
}
__device__ inline void tile_of(const LmArgs &a, int &col, int &zc) { const int tile = (int)xcd_remap(blockIdx.x, a.nblocks); zc = tile / a.cols; col = tile % a.cols; }

// whole-wave lane shifts by DPP: lane l receives the value of lane l-1 (up) / l+1 (down), 0 at the wave edge
__device__ inline double wave_up1(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ inline double wave_dn1(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// rows of the Q2 tile handled by wave w (kernels_kron.hip: equal work on the four waves of a SIMD; the two rows of a wave have one parity)
__device__ const signed char kRows64[16] = {2, 4, 6, 8, 3, 5, 7, 9, 10, 11, 12, 13, 1, 0, 15, 14};
__device__ const signed char kRows32a[16] = {2, 6, 10, 14, 3, 7, 11, 15, 18, 22, 26, 27, 19, 23, 0, 1};
__device__ const signed char kRows32b[16] = {4, 8, 12, 16, 5, 9, 13, 17, 20, 24, 28, 29, 21, 25, 30, 31};

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
constexpr unsigned kOOB = 0x80000000u;            // beyond any buffer this kernel accepts (kron_lm_apply checks the size)
__device__ inline void bload3(__amdgpu_buffer_rsrc_t r, unsigned off, double (&v)[3]) {
  const v4u t = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0); const v2u u = __builtin_amdgcn_raw_buffer_load_b64(r, off + 16u, 0, 0);
  v[0] = __hiloint2double(t.y, t.x); v[1] = __hiloint2double(t.w, t.z); v[2] = __hiloint2double(u.y, u.x);
}
__device__ inline void bstore1(__amdgpu_buffer_rsrc_t r, unsigned off, double v) { v2u u; u.x = __double2loint(v); u.y = __double2hiint(v); __builtin_amdgcn_raw_buffer_store_b64(u, r, off, 0, 0); }

struct Weights { double ll, gl, lh, gh; };   // of one plane (scalar registers)
__device__ inline Weights plane_weights(const double *__restrict__ planes, int kk) { const double *t = planes + 4 * kk; return Weights{t[0], t[1], t[2], t[3]}; }

// the fields of a vertex plane that come from component c of the window (c = 0, 1: x, y; 2: z), from the one-sided halves of its band rows:
//   m = M row, k = K row, cc = C row, t = C^T row; lo: the cell below, hi: the cell above
__device__ __forceinline__ void fields_of_component(const int c, const Weights &w, const double mlo, const double mhi, const double klo, const double khi,
                                                    const double clo, const double chi, const double tlo, const double thi, double (&f)[NF]) {
  if (c < 2) {
    f[2 * c] = fma(w.ll, mlo, w.lh * mhi);
    f[2 * c + 1] = fma(w.gl, mlo, w.gh * mhi);
    f[5 + c] = fma(w.gl, klo, w.gh * khi);
    const double s = fma(w.gl, tlo, w.gh * thi), r = fma(w.ll, clo, w.lh * chi);
    f[10 + 2 * c] = s - r; f[11 + 2 * c] = s + r;
  } else {
    f[4] = fma(w.gl, mlo, w.gh * mhi);
    f[7] = fma(fma(2.0, w.gl, w.ll), klo, fma(2.0, w.gh, w.lh) * khi);
    const double p = fma(w.ll, tlo, w.lh * thi), q = fma(w.gl, clo, w.gh * chi);
    f[8] = p - q; f[9] = p + q;
  }
}

// ---- Q2: FE_Q(2) element matrices M = (h/30) [[4,2,-1],[2,16,2],[-1,2,4]], K = (1/3h) [[7,-8,1],[-8,16,-8],[1,-8,7]], C = (1/6) [[-3,-4,1],[4,0,-4],[-1,4,3]] -----------
template <int TXN>
__device__ __forceinline__ void lm_tile_q2(const LmArgs &a, const double *__restrict__ planes, const double *__restrict__ x, double *__restrict__ y, double *Lraw, const int X0, const int tyi, const int zc) {
  constexpr int RPW = 64 / TXN, TYR = 16 * RPW, VY = TYR - 4;   // rows per wave, rows per tile, valid rows
  static_assert(TXN * TYR == kTileNodes, "tile");
  double *L = Lraw + kPad;
  const int tid = threadIdx.x;
  const int NX = a.nn[0], NY = a.nn[1], NZ = a.nn[2];
  const int Y0 = VY * tyi - 2;
  const int k0 = a.zunit * (zc * a.zq + min(zc, a.zr)), k1 = zc == a.nzc - 1 ? NZ : a.zunit * ((zc + 1) * a.zq + min(zc + 1, a.zr));

  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lx = lane % TXN;
  const int ra = RPW == 1 ? kRows64[w] : kRows32a[w], rb = RPW == 1 ? ra : kRows32b[w];
  const int r = (RPW == 2 && lane >= TXN) ? rb : ra;
  const bool odd_row = (__builtin_amdgcn_readfirstlane(ra) & 1) != 0, halo_wave = ra < 2 || ra > TYR - 3;
  const int j = Y0 + r, i = X0 + lx;
  const bool even_i = (lx & 1) == 0;
  const bool vj = j >= 0 && j < NY, vn = vj && i >= 0 && i < NX;
  const bool out = vn && lx >= 2 && lx <= TXN - 3 && !halo_wave;
  const bool bnd_xy = i == 0 || i == NX - 1 || j == 0 || j == NY - 1;

  // descriptors over the planes THIS z-chunk touches: 32-bit offsets suffice (kron_lm_apply keeps a chunk's span below 2^31 bytes)
  const unsigned nxy = (unsigned)NX * (unsigned)NY;
  const int pbase = max(k0 - 2, 0), pend = min(k1 + 2, NZ);
  const unsigned span_nodes = (unsigned)(pend - pbase) * nxy;
  const size_t base_node = (size_t)pbase * nxy;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)(x + 3 * base_node), 0, span_nodes * 24u, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)(y + 3 * base_node), 0, span_nodes * 24u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void *)(a.nodemask + base_node), 0, a.constrained ? span_nodes : 0u, 0x00020000);
  // per-lane byte offsets inside a plane; a lane without a node / an output sits beyond every buffer, and stays there when a plane's offset (< 2^31) is added
  const unsigned nxy_off = vn ? (unsigned)(j * NX + i) : kOOB;
  const unsigned ld_b = vn ? (unsigned)(j * NX + i) * 24u : kOOB, st_b = out ? (unsigned)(j * NX + i) * 24u : kOOB;

  const double mLx = i > 0 ? 1.0 : 0.0, mRx = i < NX - 1 ? 1.0 : 0.0;
  const double pe = even_i ? 1.0 : 0.0;
  const double cMx = even_i ? 4.0 * (mLx + mRx) : 16.0, cKx = even_i ? 7.0 * (mLx + mRx) : 16.0, cDx = even_i ? 3.0 * (mLx - mRx) : 0.0;
  const bool inner_y = j > 0 && j < NY - 1;
  const double nLRy = inner_y ? 2.0 : 1.0, cDyv = inner_y ? 0.0 : (j > 0 ? 3.0 : -3.0);   // vertex rows: cells on either side of the row; centre coefficients 4 | 7 times that (mid rows: 16, 16, 0 as literals)
  const LmScales &K = a.k;

  const bool mask_all = a.mask_anywhere != 0;
  auto load_plane = [&](int p, double (&v)[3], unsigned &m) {
    const bool pin = p >= 0 && p < NZ;                                   // wave-uniform
    const unsigned pl = pin ? (unsigned)(p - pbase) * nxy : kOOB;     // scalar
    bload3(rx, pin ? ld_b + pl * 24u : kOOB, v);
    const bool mk = pin && vn && (mask_all || p == 0 || p == NZ - 1 || bnd_xy);
    m = __builtin_amdgcn_raw_buffer_load_b8(rm, mk ? nxy_off + pl : kOOB, 0, 0);
  };
  auto apply_mask = [&](double (&v)[3], unsigned m) {
    if (__builtin_amdgcn_ballot_w64(m != 0) == 0) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) if (m & (1u << c)) v[c] = 0.0;
  };

  double W0[3], W1[3], W2[3], W3[3], W4[3];
  unsigned m0, m1;
  load_plane(k0 - 2, W0, m0); apply_mask(W0, m0); load_plane(k0 - 1, W1, m0); apply_mask(W1, m0); load_plane(k0, W2, m0); apply_mask(W2, m0);
  load_plane(k0 + 1, W3, m0); apply_mask(W3, m0); load_plane(k0 + 2, W4, m0); apply_mask(W4, m0);

  double dot_acc = 0.0;
  // one plane: z-stage in registers -> barrier (the previous plane's readers are done) -> LDS -> barrier -> y-stage -> x-stage -> store
  auto plane = [&](const int kk, const bool oddz, auto &&after_zstage) {
    {
      double f[NF];
      const Weights wt = plane_weights(planes, kk);
      if (!oddz) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          fields_of_component(c, wt, fma(4.0, W2[c], fma(2.0, W1[c], -W0[c])), fma(4.0, W2[c], fma(2.0, W3[c], -W4[c])), fma(7.0, W2[c], fma(-8.0, W1[c], W0[c])), fma(7.0, W2[c], fma(-8.0, W3[c], W4[c])),
                              fma(3.0, W2[c], fma(4.0, W1[c], -W0[c])), fma(-3.0, W2[c], fma(-4.0, W3[c], W4[c])), fma(3.0, W2[c], fma(-4.0, W1[c], W0[c])), fma(-3.0, W2[c], fma(4.0, W3[c], -W4[c])), f);
      } else {   // mid plane: couples to kk-1, kk, kk+1 = W2, W3, W4, all inside one layer (C row 4 (u- - u+), C^T row its negative)
        const double lam = wt.ll, G = wt.gl, l2g = fma(2.0, G, lam), cl = -(lam + G);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double t1 = W2[c] + W4[c], m = fma(16.0, W3[c], 2.0 * t1), k = fma(16.0, W3[c], -8.0 * t1), c4 = 4.0 * (W2[c] - W4[c]);
          if (c < 2) { f[2 * c] = lam * m; f[2 * c + 1] = G * m; f[5 + c] = G * k; f[10 + 2 * c] = cl * c4; f[11 + 2 * c] = (lam - G) * c4; }
          else { f[4] = G * m; f[7] = l2g * k; f[8] = cl * c4; f[9] = (G - lam) * c4; }
        }
      }
      __syncthreads();                                  // every wave has finished reading the previous plane's fields
#pragma unroll
      for (int q = 0; q < NF; ++q) L[(q * TYR + r) * TXN + lx] = f[q];
    }
    after_zstage();                                    // (the even plane issues the prefetch of the next pair here: W0, W1 are dead now)
    __syncthreads();
    if (halo_wave) return;

    const double (&xc)[3] = oddz ? W3 : W2;            // this plane's (masked) input values, for the fused x.y
    auto rest = [&](auto ODD) {
      constexpr bool odd = decltype(ODD)::value;
      struct Nb { double nm2, nm1, own, np1, np2; };
      auto ld = [&](int q, Nb &n) {
        const double *col = L + (q * TYR + r) * TXN + lx;
        n.nm1 = col[-TXN]; n.np1 = col[TXN]; n.own = col[0];
        if constexpr (!odd) { n.nm2 = col[-2 * TXN]; n.np2 = col[2 * TXN]; }
      };
      // y-bands of the integer 1D matrices: mid rows 3-point without a diagonal of C, vertex rows 5-point
      auto sM = [&](const Nb &n) { const double s1 = n.nm1 + n.np1; if constexpr (odd) return fma(2.0, s1, 16.0 * n.own); else return fma(2.0, s1, 4.0 * (nLRy * n.own)) - (n.nm2 + n.np2); };
      auto sK = [&](const Nb &n) { const double s1 = n.nm1 + n.np1; if constexpr (odd) return fma(-8.0, s1, 16.0 * n.own); else return fma(-8.0, s1, 7.0 * (nLRy * n.own)) + (n.nm2 + n.np2); };
      auto sO = [&](const Nb &n) { const double d1 = n.nm1 - n.np1; if constexpr (odd) return 4.0 * d1; else return fma(4.0, d1, n.np2 - n.nm2); };
      auto sD = [&](const Nb &n) { if constexpr (odd) return 0.0; else return cDyv * n.own; };

      auto xstage = [&](const double FK, const double FM, const double FO, const double FD) {
        const double t1 = fma(-8.0, FK, 2.0 * FM);
        const double t2 = pe * (FK - FM);
        const double pO = pe * FO;
        double sacc = fma(cKx, FK, fma(cMx, FM, cDx * FD));
        sacc += wave_up1(fma(4.0, FO, t1) + wave_up1(t2 - pO)) + wave_dn1(fma(-4.0, FO, t1) + wave_dn1(t2 + pO));
        return sacc;
      };
      const unsigned so = st_b + (unsigned)(kk - pbase) * nxy * 24u;
      auto emit = [&](int c, double v) { bstore1(ry, so + 8u * c, v); dot_acc = fma(xc[c], v, dot_acc); };

      Nb A, B;
      double XK0, XM0, XO0, XD0, XK1, XM1, XO1, XD1;
      ld(0, A); ld(1, B);                                                                   // Mz^l u_x, Mz^G u_x
      { const double OA = sO(A), OB = sO(B), DA = sD(A), DB = sD(B);
        XK0 = K.xk * fma(2.0, sM(B), sM(A)); XM0 = K.ky * sK(B);
        XO1 = K.cz * ((DB - DA) - (OA + OB)); XD1 = K.cz * ((OA - OB) + (DA + DB)); }
      ld(5, A);                                                                             // Kz^G u_x
      XM0 = fma(K.kz, sM(A), XM0);
      ld(2, A); ld(3, B);                                                                   // Mz^l u_y, Mz^G u_y
      { const double OA = sO(A), OB = sO(B), DA = sD(A), DB = sD(B);
        XK1 = K.xk * sM(B); XM1 = K.ky * fma(2.0, sK(B), sK(A));
        XO0 = K.cz * ((DA - DB) - (OA + OB)); XD0 = K.cz * ((OB - OA) + (DA + DB)); }
      ld(8, A); ld(9, B);                                                                   // coupling fields of u_z
      XO0 = fma(K.oz, sM(A), XO0); XD0 = fma(K.oz, sM(B), XD0); XM1 = fma(K.mx, sO(A) + sD(B), XM1);
      emit(0, xstage(XK0, XM0, XO0, XD0));
      __builtin_amdgcn_sched_barrier(0);
      ld(6, A);                                                                             // Kz^G u_y
      XM1 = fma(K.kz, sM(A), XM1);
      emit(1, xstage(XK1, XM1, XO1, XD1));
      __builtin_amdgcn_sched_barrier(0);
      double XK2, XM2, XO2, XD2;
      ld(4, A); ld(7, B);                                                                   // Mz^G u_z, Kz^(l+2G) u_z
      XK2 = K.xk * sM(A); XM2 = fma(K.kz, sM(B), K.ky * sK(A));
      ld(10, A); ld(11, B);                                                                 // coupling fields of u_x
      XO2 = K.oz * sM(A); XD2 = K.oz * sM(B);
      ld(12, A); ld(13, B);                                                                 // coupling fields of u_y
      XM2 = fma(K.mx, sO(A) + sD(B), XM2);
      emit(2, xstage(XK2, XM2, XO2, XD2));
    };
    if (odd_row) rest(std::true_type{}); else rest(std::false_type{});
  };

  for (int k = k0; k < k1; k += 2) {
    plane(k, false, [&] { load_plane(k + 3, W0, m0); load_plane(k + 4, W1, m1); });   // planes k-2, k-1 are no longer needed
    if (k + 1 < k1) plane(k + 1, true, [] {});
#pragma unroll
    for (int c = 0; c < 3; ++c) { const double t0 = W0[c], t1 = W1[c]; W0[c] = W2[c]; W1[c] = W3[c]; W2[c] = W4[c]; W3[c] = t0; W4[c] = t1; }
    apply_mask(W3, m0); apply_mask(W4, m1);
  }
  if (a.dot_partials) {   // deterministic workgroup reduction of x.y (fixed shuffle tree, waves summed in index order)
    if (!out) dot_acc = 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dot_acc += __shfl_xor(dot_acc, off, 64);
    __syncthreads();
    if (lane == 0) L[w] = dot_acc;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int q = 0; q < 16; ++q) t += L[q]; a.dot_partials[blockIdx.x] = t; }
  }
}

__global__ void __launch_bounds__(1024)
k_kron3_q2_lm(LmArgs a, const double *__restrict__ planes /* [nn[2]][4]: lambda_lo, G_lo, lambda_hi, G_hi */, const double *__restrict__ x, double *__restrict__ y) {
  extern __shared__ double L[];                            // [pad][14 fields][1024 nodes of the tile plane][pad]
  if (a.pcg && (a.pcg->done || a.pcg->finishing)) return;  // uniform over the grid
  int col, zc; tile_of(a, col, zc);                        // workgroup-uniform: either tile shape, never both
  if (col < a.n64 * a.nty64) lm_tile_q2<64>(a, planes, x, y, L, 60 * (col / a.nty64) - 2, col % a.nty64, zc);
  else lm_tile_q2<32>(a, planes, x, y, L, a.x0_32, col - a.n64 * a.nty64, zc);
}

// ---- Q1: M = (h/6) [[2,1],[1,2]], K = (1/h) [[1,-1],[-1,1]], C = (1/2) [[-1,-1],[1,1]]; every plane is a vertex plane, 3-plane window ----------------------------
template <int TXN>
__device__ __forceinline__ void lm_tile_q1(const LmArgs &a, const double *__restrict__ planes, const double *__restrict__ x, double *__restrict__ y, double *Lraw, const int X0, const int tyi, const int zc) {
  constexpr int RPW = 64 / TXN, TYR = 16 * RPW, VY = TYR - 2;
  double *L = Lraw + kPad;
  const int tid = threadIdx.x;
  const int NX = a.nn[0], NY = a.nn[1], NZ = a.nn[2];
  const int Y0 = VY * tyi - 1;
  const int k0 = a.zunit * (zc * a.zq + min(zc, a.zr)), k1 = zc == a.nzc - 1 ? NZ : a.zunit * ((zc + 1) * a.zq + min(zc + 1, a.zr));
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lx = lane % TXN;
  const int r = RPW == 1 ? w : w + 16 * (lane / TXN);
  const bool halo_wave = RPW == 1 && (w == 0 || w == 15);        // (two rows per wave: halo rows share waves with valid rows)
  const int j = Y0 + r, i = X0 + lx;
  const bool vj = j >= 0 && j < NY, vn = vj && i >= 0 && i < NX;
  const bool out = vn && lx >= 1 && lx <= TXN - 2 && r >= 1 && r <= TYR - 2;
  const bool bnd_xy = i == 0 || i == NX - 1 || j == 0 || j == NY - 1;
  const double mLx = i > 0 ? 1.0 : 0.0, mRx = i < NX - 1 ? 1.0 : 0.0, mLy = j > 0 ? 1.0 : 0.0, mRy = j < NY - 1 ? 1.0 : 0.0;
  const double cMx = 2.0 * (mLx + mRx), cKx = mLx + mRx, cDx = mLx - mRx, cMy = 2.0 * (mLy + mRy), cKy = mLy + mRy, cDy = mLy - mRy;
  const LmScales &K = a.k;

  const unsigned nxy = (unsigned)NX * (unsigned)NY;
  const int pbase = max(k0 - 1, 0), pend = min(k1 + 1, NZ);
  const unsigned span_nodes = (unsigned)(pend - pbase) * nxy;
  const size_t base_node = (size_t)pbase * nxy;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)(x + 3 * base_node), 0, span_nodes * 24u, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)(y + 3 * base_node), 0, span_nodes * 24u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void *)(a.nodemask + base_node), 0, a.constrained ? span_nodes : 0u, 0x00020000);
  const unsigned nxy_off = vn ? (unsigned)(j * NX + i) : kOOB, out_off = out ? (unsigned)(j * NX + i) : kOOB;
  const bool mask_all = a.mask_anywhere != 0;
  auto load_plane = [&](int p, double (&v)[3], unsigned &m) {
    const bool pin = p >= 0 && p < NZ;
    const unsigned node = (unsigned)(p - pbase) * nxy + nxy_off;
    bload3(rx, (pin && vn) ? node * 24u : kOOB, v);
    const bool mk = pin && vn && (mask_all || p == 0 || p == NZ - 1 || bnd_xy);
    m = __builtin_amdgcn_raw_buffer_load_b8(rm, mk ? node : kOOB, 0, 0);
  };
  auto apply_mask = [&](double (&v)[3], unsigned m) {
    if (__builtin_amdgcn_ballot_w64(m != 0) == 0) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) if (m & (1u << c)) v[c] = 0.0;
  };
  double W0[3], W1[3], W2[3];   // planes k-1, k, k+1
  unsigned m0;
  load_plane(k0 - 1, W0, m0); apply_mask(W0, m0); load_plane(k0, W1, m0); apply_mask(W1, m0); load_plane(k0 + 1, W2, m0); apply_mask(W2, m0);

  struct Nb { double nm1, own, np1; };
  auto ld = [&](int q, Nb &n) { const double *col = L + (q * TYR + r) * TXN + lx; n.nm1 = col[-TXN]; n.np1 = col[TXN]; n.own = col[0]; };
  auto sM = [&](const Nb &n) { return fma(cMy, n.own, n.nm1 + n.np1); };
  auto sK = [&](const Nb &n) { return fma(cKy, n.own, -(n.nm1 + n.np1)); };
  auto sO = [&](const Nb &n) { return n.nm1 - n.np1; };
  auto sD = [&](const Nb &n) { return cDy * n.own; };
  double dot_acc = 0.0;

  for (int kk = k0; kk < k1; ++kk) {
    {
      double f[NF];
      const Weights wt = plane_weights(planes, kk);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double klo = W1[c] - W0[c], khi = W1[c] - W2[c];
        fields_of_component(c, wt, fma(2.0, W1[c], W0[c]), fma(2.0, W1[c], W2[c]), klo, khi, W0[c] + W1[c], -(W1[c] + W2[c]), klo, -khi, f);
      }
      __syncthreads();                                  // every wave has finished reading the previous plane's fields
#pragma unroll
      for (int q = 0; q < NF; ++q) L[(q * TYR + r) * TXN + lx] = f[q];
    }
    const double xc[3] = {W1[0], W1[1], W1[2]};   // this plane's (masked) input values
    unsigned mp; load_plane(kk + 2, W0, mp);      // plane k-1 is no longer needed: prefetch plane k+2 into its registers
    __syncthreads();

    if (!halo_wave) {
      auto xstage = [&](const double FK, const double FM, const double FO, const double FD) {
        const double t1 = FM - FK;
        return fma(cKx, FK, fma(cMx, FM, cDx * FD)) + wave_up1(t1 + FO) + wave_dn1(t1 - FO);   // from i-1 and i+1
      };
      const unsigned so = out ? ((unsigned)(kk - pbase) * nxy + out_off) * 24u : kOOB;
      auto emit = [&](int c, double v) { bstore1(ry, so + 8u * c, v); dot_acc = fma(xc[c], v, dot_acc); };
      Nb A, B;
      double XK0, XM0, XO0, XD0, XK1, XM1, XO1, XD1;
      ld(0, A); ld(1, B);
      { const double OA = sO(A), OB = sO(B), DA = sD(A), DB = sD(B);
        XK0 = K.xk * fma(2.0, sM(B), sM(A)); XM0 = K.ky * sK(B);
        XO1 = K.cz * ((DB - DA) - (OA + OB)); XD1 = K.cz * ((OA - OB) + (DA + DB)); }
      ld(5, A);
      XM0 = fma(K.kz, sM(A), XM0);
      ld(2, A); ld(3, B);
      { const double OA = sO(A), OB = sO(B), DA = sD(A), DB = sD(B);
        XK1 = K.xk * sM(B); XM1 = K.ky * fma(2.0, sK(B), sK(A));
        XO0 = K.cz * ((DA - DB) - (OA + OB)); XD0 = K.cz * ((OB - OA) + (DA + DB)); }
      ld(8, A); ld(9, B);
      XO0 = fma(K.oz, sM(A), XO0); XD0 = fma(K.oz, sM(B), XD0); XM1 = fma(K.mx, sO(A) + sD(B), XM1);
      emit(0, xstage(XK0, XM0, XO0, XD0));
      ld(6, A);
      XM1 = fma(K.kz, sM(A), XM1);
      emit(1, xstage(XK1, XM1, XO1, XD1));
      double XK2, XM2, XO2, XD2;
      ld(4, A); ld(7, B);
      XK2 = K.xk * sM(A); XM2 = fma(K.kz, sM(B), K.ky * sK(A));
      ld(10, A); ld(11, B);
      XO2 = K.oz * sM(A); XD2 = K.oz * sM(B);
      ld(12, A); ld(13, B);
      XM2 = fma(K.mx, sO(A) + sD(B), XM2);
      emit(2, xstage(XK2, XM2, XO2, XD2));
    }
    // rotate the window by one plane; the prefetched plane gets its Dirichlet columns zeroed as it enters
#pragma unroll
    for (int c = 0; c < 3; ++c) { const double t0 = W0[c]; W0[c] = W1[c]; W1[c] = W2[c]; W2[c] = t0; }
    apply_mask(W2, mp);
  }
  if (a.dot_partials) {
    if (!out) dot_acc = 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dot_acc += __shfl_xor(dot_acc, off, 64);
    __syncthreads();
    if (lane == 0) L[w] = dot_acc;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int q = 0; q < 16; ++q) t += L[q]; a.dot_partials[blockIdx.x] = t; }
  }
}

__global__ void __launch_bounds__(1024)
k_kron3_q1_lm(LmArgs a, const double *__restrict__ planes /* [nn[2]][4]: lambda_lo, G_lo, lambda_hi, G_hi */, const double *__restrict__ x, double *__restrict__ y) {
  extern __shared__ double L[];
  if (a.pcg && (a.pcg->done || a.pcg->finishing)) return;
  int col, zc; tile_of(a, col, zc);
  if (col < a.n64 * a.nty64) lm_tile_q1<64>(a, planes, x, y, L, 62 * (col / a.nty64) - 1, col % a.nty64, zc);
  else lm_tile_q1<32>(a, planes, x, y, L, a.x0_32, col - a.n64 * a.nty64, zc);
}

constexpr size_t kLdsBytes = (size_t)(NF * kTileNodes + 2 * kPad) * sizeof(double);

}  // namespace

void kron_lm_prepare_device() {
  PORO_HIP(hipFuncSetAttribute((const void *)k_kron3_q2_lm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
  PORO_HIP(hipFuncSetAttribute((const void *)k_kron3_q1_lm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
}

// planes: the device copy of moduli_plane_table for this box, [k_u n_z + 1][4].  Everything else as kron_apply (3D, plain operator)
int kron_lm_apply(hipStream_t s, const MfArgs &m, const double *planes, const double *x, double *y, bool constrained, int n_cus, double *dot_partials, hipEvent_t ev0, hipEvent_t ev1,
                  const PcgScalars *pcg) {
  const int ku = m.k_u;
  if (m.dim != 3 || (ku != 1 && ku != 2) || !planes) throw Error("structured operator for layered moduli: 3D boxes of degree 1 or 2 with a plane table");
  LmArgs a{};
  for (int d = 0; d < 3; ++d) a.nn[d] = ku * m.box.n[d] + 1;
  // the tiling of kron_apply: (64 lanes x 16 rows) and (32 x 32) tiles, one round of z-chunks over the chip
  const int vx64 = ku == 2 ? 60 : 62, vx32 = ku == 2 ? 28 : 30, vy64 = ku == 2 ? 12 : 14, vy32 = ku == 2 ? 28 : 30, halo = ku == 2 ? 2 : 1;
  a.n64 = a.nn[0] / vx64; const int rem = a.nn[0] - vx64 * a.n64;
  a.has32 = 0;
  if (rem > vx32) a.n64 += 1; else if (rem > 0) a.has32 = 1;
  a.x0_32 = vx64 * a.n64 - halo;
  a.nty64 = (a.nn[1] + vy64 - 1) / vy64; a.nty32 = (a.nn[1] + vy32 - 1) / vy32;
  const int cols = a.n64 * a.nty64 + a.has32 * a.nty32;
  a.zunit = ku == 2 ? 2 : 1;
  const int units = a.nn[2] / a.zunit;
  int min_chunk = 8;
  if ((int64_t)cols * ((units * a.zunit + 7) / 8) < n_cus) min_chunk = 4;
  const int upc = std::max(1, min_chunk / a.zunit);
  int nzc = n_cus / cols; if (nzc > (units + upc - 1) / upc) nzc = (units + upc - 1) / upc; if (nzc < 1) nzc = 1;
  { const int64_t plane_bytes = (int64_t)a.nn[0] * a.nn[1] * 24, max_planes = (((int64_t)1 << 31) - 1) / plane_bytes - 2 * halo - 3;
    if (max_planes < 2 * a.zunit) throw Error("structured operator: an x-y plane of the box is too large for 32-bit buffer offsets");
    const int need = (int)((a.nn[2] + max_planes - 1) / max_planes);
    if (nzc < need) nzc = std::min(need, units); }
  a.nzc = nzc; a.zq = units / nzc; a.zr = units % nzc;
  a.nA = a.n64 * a.nty64 * a.nzc; a.nblocks = a.nA + a.has32 * a.nty32 * a.nzc; a.cols = cols;
  const double mdiv = ku == 2 ? 30.0 : 6.0, kmul = ku == 2 ? 1.0 / 3.0 : 1.0, sC = ku == 2 ? 1.0 / 6 : 0.5;   // scales of the integer 1D matrices
  const double sM[3] = {m.box.h[0] / mdiv, m.box.h[1] / mdiv, m.box.h[2] / mdiv}, sK[3] = {kmul / m.box.h[0], kmul / m.box.h[1], kmul / m.box.h[2]};
  a.k.xk = sK[0] * sM[1] * sM[2]; a.k.ky = sM[0] * sK[1] * sM[2]; a.k.kz = sM[0] * sM[1] * sK[2];
  a.k.cz = sC * sC * sM[2]; a.k.oz = sC * sM[1] * sC; a.k.mx = sM[0] * sC * sC;
  a.nodemask = m.nodemask; a.constrained = constrained ? 1 : 0; a.mask_anywhere = m.mask_anywhere;
  const int nblk = a.nblocks;
  const bool fuse = dot_partials && nblk <= kMaxPartials / 2;      // one partial slot per workgroup (negative return value = "no partials written")
  a.dot_partials = fuse ? dot_partials : nullptr; a.pcg = pcg;
  if (ku == 2) hipExtLaunchKernelGGL(k_kron3_q2_lm, dim3((unsigned)nblk), dim3(1024), kLdsBytes, s, ev0, ev1, 0, a, planes, x, y);
  else hipExtLaunchKernelGGL(k_kron3_q1_lm, dim3((unsigned)nblk), dim3(1024), kLdsBytes, s, ev0, ev1, 0, a, planes, x, y);
  return (dot_partials && !fuse) ? -nblk : nblk;
}

}  // namespace poro
