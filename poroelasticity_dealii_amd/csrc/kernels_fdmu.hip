// Block fast-diagonalisation preconditioner of the DISPLACEMENT system (K-prec, SURVEY 8f-1 "a stronger preconditioner") on uniform
// boxes (gfx950, wave64, fp64 / fp32 MFMA).
//
// On a box the diagonal blocks of A_u (PoroElasticDisplacementSolver.h:230-242, one block per displacement component c) are
//   A_cc = sum_d coef(c,d) (K_d in direction d) (x) (M_e in the other directions),   coef = lambda + 2G (d == c) | G (d != c),
// with the 1D FE_Q(k_u) mass / stiffness matrices M_d, K_d; a Dirichlet condition on component c over a whole face removes the end
// node of that direction from the 1D matrices of component c, so the structure survives the constraints.  With the generalised 1D
// eigen-decompositions K S = M S Lambda, S^T M S = I (host, once per mesh; one set per component because the end conditions differ)
//   A_cc^-1 = (Sx (x) Sy (x) Sz) diag(sum_d coef(c,d) lam_d)^-1 (Sx (x) Sy (x) Sz)^T   EXACTLY.
// z = blockdiag(A_cc)^-1 g is spectrally equivalent to A_u^-1 (Korn): CG needs ~20 iterations independent of h instead of O(1/h)
// with Jacobi (245 at BASELINE config 4).  The off-diagonal blocks A_ab (products of first-derivative matrices) are not separable and
// stay in the Krylov iteration.
//
// One application = 2 dim dense (n_d x n_d) transforms along the grid lines of a [component][z][y][x] array: GEMM-shaped work
// (2 x 3 x 6 x 145^4 = 1.6e10 flop at config 4), so it runs on the matrix cores.  One kernel serves every pass:
//   load a panel of 32 grid lines (all points of each line) into LDS -> D = T1 * panel on v_mfma_f64_16x16x4_f64 (T as the A operand,
//   streamed from L2 in MFMA fragment order, 512 contiguous bytes per wave and k-step; panel columns as the B operand from LDS)
//   -> [last direction only: scale by the inverse eigenvalue sums, write back to LDS, second GEMM with T2 = S] -> LDS -> coalesced store.
// The first pass reads the node-interleaved residual (dof = node * dim + c), the last pass writes the interleaved z; in between the
// data are component-planar.  Passes: x, y, z (forward + scaling + backward fused), y, x  = 5 sweeps over the vector in 3D.
// Rows / columns of constrained end nodes are zero in S, so z = 0 on Dirichlet dofs (they are inert inside PCG anyway).
#include "common.hpp"
#include "fdm_tables.hpp"
#include <cmath>
#include <limits>
#include <type_traits>

namespace poro {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
template <class T> struct Mfma;
template <> struct Mfma<double> { typedef v4d acc_t; static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); } };
template <> struct Mfma<float> { typedef v4f acc_t; static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); } };

constexpr int kNT = 32;        // grid lines per panel (two 16-column MFMA tiles)
constexpr int kLdK = kNT + 16; // LDS row stride of a [k][line] panel: the four k-rows of a B fragment land in disjoint banks
constexpr int kThreads = 256;  // 4 waves: wave w owns column tile w & 1 and the output row tiles of half w >> 1

struct FdmuPass {
  int nK;               // points per line (= output rows)
  int MT, KK;           // 16-row output tiles, 4-deep k-steps (both ceil)
  int64_t SI;           // element stride along the line: 1 (x), nx (y), nx ny (z)
  int64_t n_lines;      // lines per component
  int64_t comp_stride;  // planar arrays: elements per component
  int ncomp;
  int in_interleaved, out_interleaved;   // array layout: element (line point e, component c) at e * ncomp + c instead of c * comp_stride + e
  int x_layout;         // 1: LDS panel stored [line][k] (contiguous lines: the x direction), 0: [k][line]
  int ld_line;          // x_layout: LDS stride between lines
  // fused scaling (last direction): D(m, line) /= kd * lam_d[m] + k0 * lam0[i] + k1 * lam1[j], (i, j) = grid position of the line
  int fused; int n0; int64_t col0, col_total; double kd[3], k0[3], k1[3];
  int reg_form;         // 1: register-panel kernel (T1 / T2 point at the chunked fragment order of k_fdmu_reg)
  int split;            // 1: even / odd form (k_fdmu_split): every component's 1D eigenvectors are symmetric or antisymmetric about the line's centre
  int split_dir;        // split, not fused: 0 forward (nodes -> modes), 1 backward
  int n_even[3];        // split: even modes per component (mode order along the line: even modes first, then the odd ones)
  int blk;              // split form for lines of more than 160 points (k_fdmu_blk): the output rows are produced in blocks of 80 per parity, the transform matrix is
  int blk_kk[3], blk_nch[3], blk_mb[3];   //   packed [row block][chunk]...; per component: k-steps, chunks per row block and row blocks of THIS pass (forward / backward differ)
  int scale_on_load;    // blk backward pass of the last direction: the coefficients are divided by the eigenvalue sums as they are loaded
  const void *T1[3], *T2[3];             // per component: transform matrices in MFMA fragment order [MT][KK][64]
  const double *lam_d[3], *lam0[3], *lam1[3];
};

// element index of point k of line n inside one component's grid
__device__ __forceinline__ int64_t line_base(const FdmuPass &P, int64_t n) { const int64_t o = n / P.SI; return o * P.SI * P.nK + (n - o * P.SI); }

template <class TC, class TIn, class TOut, int MTH>
__global__ void __launch_bounds__(kThreads)
k_fdmu_pass(FdmuPass P, const TIn *__restrict__ in, TOut *__restrict__ out) {
  extern __shared__ double lds_raw[];
  TC *L = reinterpret_cast<TC *>(lds_raw);
  typedef typename Mfma<TC>::acc_t acc_t;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kNT;
  const int rows = P.KK * 4 > P.MT * 16 ? P.KK * 4 : P.MT * 16;      // panel rows: k (input) or m (output), zero padded
  const int s_n = P.x_layout ? P.ld_line : 1, s_k = P.x_layout ? 1 : kLdK;

  // ---- load the panel: element (k, line) -> L[line * s_n + k * s_k]; padded rows and lines are zero ----
  if (P.x_layout) {
    // lines are contiguous in memory (planar) or ncomp-strided (interleaved): run along k
    const int total = kNT * rows;
    for (int idx = tid; idx < total; idx += kThreads) {
      const int ln = idx / rows, k = idx - ln * rows;
      const int64_t n = n0 + ln;
      TC v = 0;
      if (k < P.nK && n < P.n_lines) {
        const int64_t e = n * P.nK + k;
        v = (TC)(P.in_interleaved ? in[e * P.ncomp + c] : in[(int64_t)c * P.comp_stride + e]);
      }
      L[ln * s_n + k] = v;
    }
  } else {
    const int ln = tid & (kNT - 1);
    const int64_t n = n0 + ln;
    const bool lv = n < P.n_lines;
    const int64_t base = (int64_t)c * P.comp_stride + (lv ? line_base(P, n) : 0);
    for (int k = tid / kNT; k < rows; k += kThreads / kNT) L[k * kLdK + ln] = (lv && k < P.nK) ? (TC)in[base + (int64_t)k * P.SI] : (TC)0;
  }
  __syncthreads();

  const int nt = w & 1, mh = w >> 1;
  const int i16 = lane & 15, kq = lane >> 4;
  const TC *Bp = L + (nt * 16 + i16) * s_n + kq * s_k;       // B fragment of k-step kk: Bp[4 kk s_k]
  acc_t acc[MTH];

  auto gemm = [&](const TC *__restrict__ Tf) {
#pragma unroll
    for (int t = 0; t < MTH; ++t) acc[t] = acc_t{0, 0, 0, 0};
    const TC *Ap = Tf + ((int64_t)(mh * MTH) * P.KK) * 64 + lane;   // fragment (m-tile, kk) at ((mt * KK) + kk) * 64 + lane
    int kk = 0;
    for (; kk + 4 <= P.KK; kk += 4) {          // 4 k-steps per trip, every operand load issued before the first MFMA
      TC a[4][MTH], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        b[u] = Bp[(kk + u) * 4 * s_k];
#pragma unroll
        for (int t = 0; t < MTH; ++t) a[u][t] = (mh * MTH + t < P.MT) ? Ap[((int64_t)t * P.KK + kk + u) * 64] : (TC)0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < MTH; ++t) acc[t] = Mfma<TC>::run(a[u][t], b[u], acc[t]);
    }
    for (; kk < P.KK; ++kk) {
      const TC b = Bp[kk * 4 * s_k];
#pragma unroll
      for (int t = 0; t < MTH; ++t) { const TC a = (mh * MTH + t < P.MT) ? Ap[((int64_t)t * P.KK + kk) * 64] : (TC)0; acc[t] = Mfma<TC>::run(a, b, acc[t]); }
    }
  };
  // D fragment -> LDS, column lane & 15; the row of register q differs by MFMA: (lane >> 4) + 4 q for v_mfma_f64_16x16x4_f64, 4 (lane >> 4) + q for
  // v_mfma_f32_16x16x4_f32 (fp32 transforms)
  auto acc_to_lds = [&](bool scale) {
    double base = 0; bool lvalid = true;
    if (scale) {
      const int64_t col = P.col0 + n0 + nt * 16 + i16;           // global line index = (j, i) grid position
      lvalid = n0 + nt * 16 + i16 < P.n_lines && col < P.col_total;
      if (lvalid) {
        if (P.lam1[c]) { const int64_t j = col / P.n0; base = P.k0[c] * P.lam0[c][col - j * P.n0] + P.k1[c] * P.lam1[c][j]; }
        else if (P.lam0[c]) base = P.k0[c] * P.lam0[c][col];
      }
    }
#pragma unroll
    for (int t = 0; t < MTH; ++t) {
      const int mt = mh * MTH + t;
      if (mt >= P.MT) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = mt * 16 + (std::is_same<TC, double>::value ? kq + 4 * q : 4 * kq + q);
        double v = (double)acc[t][q];
        if (scale) v = (lvalid && m < P.nK) ? v / (base + P.kd[c] * P.lam_d[c][m]) : 0.0;   // padded / constrained modes carry lam = inf
        L[(nt * 16 + i16) * s_n + m * s_k] = (TC)v;
      }
    }
  };

  gemm(reinterpret_cast<const TC *>(P.T1[c]));
  __syncthreads();                       // everybody has finished reading the input panel
  acc_to_lds(P.fused != 0);
  if (P.fused) {
    // rows >= 16 MT of the panel still hold input data; the second GEMM's k runs to 4 KK <= rows: clear what the first result did not cover
    for (int idx = tid; idx < (rows - P.MT * 16) * kNT; idx += kThreads) { const int k = P.MT * 16 + idx / kNT, ln = idx % kNT; L[ln * s_n + k * s_k] = 0; }
    __syncthreads();
    gemm(reinterpret_cast<const TC *>(P.T2[c]));
    __syncthreads();
    acc_to_lds(false);
  }
  __syncthreads();

  // ---- store the panel (rows m < nK) ----
  if (P.x_layout) {
    const int total = kNT * P.nK;
    for (int idx = tid; idx < total; idx += kThreads) {
      const int ln = idx / P.nK, m = idx - ln * P.nK;
      const int64_t n = n0 + ln;
      if (n >= P.n_lines) continue;
      const int64_t e = n * P.nK + m;
      const TC v = L[ln * s_n + m];
      if (P.out_interleaved) out[e * P.ncomp + c] = (TOut)v; else out[(int64_t)c * P.comp_stride + e] = (TOut)v;
    }
  } else {
    const int ln = tid & (kNT - 1);
    const int64_t n = n0 + ln;
    if (n < P.n_lines) {
      const int64_t base = (int64_t)c * P.comp_stride + line_base(P, n);
      for (int m = tid / kNT; m < P.nK; m += kThreads / kNT) out[base + (int64_t)m * P.SI] = (TOut)L[m * kLdK + ln];
    }
  }
}

// ---- register-panel form (lines of <= 160 points, fp64): no LDS traffic for the data at all ------------------------------------------
// A wave owns 16 grid lines.  Their points go straight from global memory into MFMA B-fragment registers (lane (j, kq) holds points
// k = 4 kk + kq of line j for every k-step kk: <= 40 doubles), the transform matrix streams through LDS in chunks of 4 k-steps shared by
// the 4 waves of the workgroup (double buffered, one barrier per chunk, 16-byte LDS reads feeding two MFMAs each), and the D fragments are
// stored from the accumulators.  The D layout of v_mfma_f64_16x16x4_f64 (register q of a lane = row kq + 4 q of the tile, column j) IS the
// B layout of the next GEMM (k-step 4 mt + q of the same lane), so the fused last-direction pass chains its two GEMMs without moving data.
template <int NCH> struct RegGeom { static constexpr int MTP = (NCH + 1) / 2, MT = 2 * MTP, KKP = 4 * NCH, CHUNK = 4 * MTP * 128; };

// MODE 0: data as the B operand (y / z passes: 16 consecutive lines per tile are contiguous in memory, loads and stores run in 128-byte pieces);
// MODE 1: the same with the scaling and the second GEMM fused (last direction); MODE 2: data as the A operand (x passes: the SAME registers,
// only the operand order of the MFMA changes, and D comes out transposed - lane = point of the line - so the stores are contiguous along x).
// The data fragments of chunk ch + kAhead are requested while chunk ch multiplies (the loads stay behind the chunk's barrier).
template <int NCH, int MODE>
__global__ void __launch_bounds__(kThreads, MODE == 0 ? 1 : 2)   // (measured per mode: the register cap of two waves per SIMD pays for the fused and the x passes only)
k_fdmu_reg(FdmuPass P, const double *__restrict__ in, double *__restrict__ out) {
  typedef RegGeom<NCH> Gm;
  constexpr int kAhead = NCH < 3 ? NCH : 3;
  __shared__ double LT[2][Gm::CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y, j = lane & 15, kq = lane >> 4;
  const int64_t n_tile = (int64_t)blockIdx.x * 64 + w * 16;
  const int64_t n = n_tile + j;
  const bool valid = n < P.n_lines;
  // element (k, line n) of the input / output arrays at base + k * stride.  Loads are never predicated: lines behind the end re-read the
  // last line and points behind the line's end re-read its last point (finite values that only meet zero columns of T or are never stored)
  const int64_t nc = valid ? n : P.n_lines - 1;
  const int64_t lb = P.SI == 1 ? nc * P.nK : line_base(P, nc);
  const int64_t in_stride = P.in_interleaved ? P.SI * P.ncomp : P.SI, out_stride = P.out_interleaved ? P.SI * P.ncomp : P.SI;
  const double *in_lane = in + (P.in_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb);
  const int k_last = P.nK - 1;

  double b[Gm::KKP];
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int kk = 4 * ch + u; const int k = min(4 * kk + kq, k_last); b[kk] = in_lane[(int64_t)k * in_stride]; }
  };
#pragma unroll
  for (int ch = 0; ch < kAhead; ++ch) load_chunk(ch);

  v4d acc[Gm::MT];
  // D = T * B (or B^T * T^T for MODE 2) with T in chunked fragment order [chunk][k-step in chunk][tile pair][lane][2]
  auto gemm = [&](const double *__restrict__ Tg, double (&bb)[Gm::KKP], const bool stream_b, const bool swapped) {
#pragma unroll
    for (int t = 0; t < Gm::MT; ++t) acc[t] = v4d{0, 0, 0, 0};
    constexpr int PER = Gm::CHUNK / 2 / kThreads;   // double2 per thread and chunk = MTP
    double2 stage[PER];
    const double2 *src = reinterpret_cast<const double2 *>(Tg);
#pragma unroll
    for (int i = 0; i < PER; ++i) reinterpret_cast<double2 *>(LT[0])[tid + i * kThreads] = src[tid + i * kThreads];
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (ch + 1 < NCH) {
#pragma unroll
        for (int i = 0; i < PER; ++i) stage[i] = src[(int64_t)(ch + 1) * (Gm::CHUNK / 2) + tid + i * kThreads];
      }
      if (stream_b && ch + kAhead < NCH) load_chunk(ch + kAhead);
      const double2 *La = reinterpret_cast<const double2 *>(LT[ch & 1]) + lane;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = 4 * ch + u;
        if (ch + 1 < NCH || u == 0 || kk < P.KK) {         // wave-uniform, last chunk only: k-steps behind the line length are skipped
#pragma unroll
          for (int p = 0; p < Gm::MTP; ++p) {
            const double2 a = La[(u * Gm::MTP + p) * 64];
            if (swapped) {
              acc[2 * p] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[kk], a.x, acc[2 * p], 0, 0, 0);
              acc[2 * p + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[kk], a.y, acc[2 * p + 1], 0, 0, 0);
            } else {
              acc[2 * p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bb[kk], acc[2 * p], 0, 0, 0);
              acc[2 * p + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bb[kk], acc[2 * p + 1], 0, 0, 0);
            }
          }
        }
      }
      if (ch + 1 < NCH) {
#pragma unroll
        for (int i = 0; i < PER; ++i) reinterpret_cast<double2 *>(LT[(ch + 1) & 1])[tid + i * kThreads] = stage[i];
      }
      __syncthreads();
    }
  };

  gemm(reinterpret_cast<const double *>(P.T1[c]), b, true, MODE == 2);
  if constexpr (MODE == 1) {
    double base = 0;
    const int64_t col = min(P.col0 + nc, P.col_total - 1);     // (lines behind the end: any valid column, the result is never stored)
    if (P.lam1[c]) { const int64_t jj = col / P.n0; base = P.k0[c] * P.lam0[c][col - jj * P.n0] + P.k1[c] * P.lam1[c][jj]; }
    else if (P.lam0[c]) base = P.k0[c] * P.lam0[c][col];
    double b2[Gm::KKP];
    const double *lam_lane = P.lam_d[c]; const double kdc = P.kd[c];
#pragma unroll
    for (int mt = 0; mt < NCH; ++mt) {        // D register (mt, q) of this lane = B operand of k-step 4 mt + q.  (Tiles come in pairs: with an odd number of chunks the last tile, mt = NCH, holds rows
                                              //  behind the line's end only - exact zeros - and b2 has no k-steps for it: looping to MT wrote past b2, which broke lines of 33-48, 65-80, ... points in this
                                              //  non-symmetric form until round 3)
      double den[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) den[q] = fma(kdc, lam_lane[min(16 * mt + kq + 4 * q, k_last)], base);   // removed modes carry lam = inf -> factor 0
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // reciprocal by v_rcp_f64 + one Newton step (full division sequences would cost a quarter of the GEMM); den = inf gives exactly 0
        double r = __builtin_amdgcn_rcp(den[q]);
        r = den[q] < 1e300 ? fma(r, fma(-den[q], r, 1.0), r) : 0.0;
        b2[4 * mt + q] = acc[mt][q] * r;       // rows behind the line's end are exact zeros of T
      }
      __builtin_amdgcn_sched_barrier(0);       // keep the eigenvalue loads of the next tile from piling up in registers
    }
    gemm(reinterpret_cast<const double *>(P.T2[c]), b2, false, false);
  }
  if constexpr (MODE == 2) {
    // transposed D: lane j = point 16 t + j of the line, register q = line kq + 4 q of the tile (x direction: SI == 1)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t nl = n_tile + kq + 4 * q;
      if (nl >= P.n_lines) continue;
      const int64_t ob = P.out_interleaved ? nl * P.nK * P.ncomp + c : (int64_t)c * P.comp_stride + nl * P.nK;
#pragma unroll
      for (int t = 0; t < Gm::MT; ++t) { const int m = 16 * t + j; if (m < P.nK) out[ob + (int64_t)m * out_stride] = acc[t][q]; }
    }
  } else if (valid) {
    const int64_t out_base = P.out_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb;
#pragma unroll
    for (int t = 0; t < Gm::MT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int m = 16 * t + kq + 4 * q; if (m < P.nK) out[out_base + (int64_t)m * out_stride] = acc[t][q]; }
  }
}

// ---- even / odd form ---------------------------------------------------------------------------------------------------------------
// On a uniform mesh with the same end condition at both ends the 1D matrices are persymmetric, so every eigenvector is symmetric or
// antisymmetric about the centre of the line.  With e_k = x_k + x_{n-1-k}, o_k = x_k - x_{n-1-k} (k in the lower half, the centre node kept as
// it is) the forward transform splits into two half-size products (even modes from e, odd modes from o) and the backward transform into two
// half-size products followed by x_k = a_k + b_k, x_{n-1-k} = a_k - b_k: HALF the MFMA work of the full transform.  A lane loads point
// 4 kk + kq of its line AND its mirror image, so the butterflies stay inside the lane; the two products of a pass run as the two MFMAs fed by
// one 16-byte LDS read (tile pair p = even tile p, odd tile p) and share the chunked streaming of k_fdmu_reg.  Modes are stored along the line
// with the even ones first; the eigenvalue arrays are permuted to match.  MODE 0: forward, 1: backward, 2: forward + scaling + backward.
template <int NCH> struct SplitGeom { static constexpr int P = NCH, KKP = 4 * NCH, CHUNK = 4 * NCH * 128; };

template <int NCH, int MODE>
__global__ void __launch_bounds__(kThreads, 2)
k_fdmu_split(FdmuPass P, const double *__restrict__ in, double *__restrict__ out) {
  typedef SplitGeom<NCH> Gm;
  constexpr int kAhead = NCH < 2 ? NCH : 2;
  __shared__ double LT[2][Gm::CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y, j = lane & 15, kq = lane >> 4;
  const int64_t n = (int64_t)blockIdx.x * 64 + w * 16 + j;
  const bool valid = n < P.n_lines;
  const int64_t nc = valid ? n : P.n_lines - 1;
  const int64_t lb = P.SI == 1 ? nc * P.nK : line_base(P, nc);
  const int64_t in_stride = P.in_interleaved ? P.SI * P.ncomp : P.SI, out_stride = P.out_interleaved ? P.SI * P.ncomp : P.SI;
  const double *in_lane = in + (P.in_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb);
  double *out_lane = out + (P.out_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb);
  const int nn = P.nK, h = (nn + 1) / 2, ne = P.n_even[c], k_last = nn - 1;
  const int KK = (h + 3) / 4;

  // first operand pair: forward = (e, o) from a point and its mirror image; backward = (even, odd) coefficient groups
  double b0[Gm::KKP], b1[Gm::KKP];
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = 4 * ch + u, k = 4 * kk + kq;
      if (MODE == 1) {
        b0[kk] = in_lane[(int64_t)min(k, k_last) * in_stride];
        b1[kk] = in_lane[(int64_t)min(ne + k, k_last) * in_stride];
      } else {
        const int kc = min(k, h - 1), km = k_last - kc;
        const double lo = in_lane[(int64_t)kc * in_stride], hi = in_lane[(int64_t)km * in_stride];
        b0[kk] = km == kc ? lo : lo + hi;       // the centre node of an odd line is its own mirror image
        b1[kk] = lo - hi;
      }
    }
  };
#pragma unroll
  for (int ch = 0; ch < kAhead; ++ch) load_chunk(ch);

  v4d acc[2 * Gm::P];
  auto gemm = [&](const double *__restrict__ Tg, double (&be)[Gm::KKP], double (&bo)[Gm::KKP], const bool stream_b) {
#pragma unroll
    for (int t = 0; t < 2 * Gm::P; ++t) acc[t] = v4d{0, 0, 0, 0};
    constexpr int PER = Gm::CHUNK / 2 / kThreads;
    double2 stage[PER > 0 ? PER : 1];
    const double2 *src = reinterpret_cast<const double2 *>(Tg);
    for (int i = tid; i < Gm::CHUNK / 2; i += kThreads) reinterpret_cast<double2 *>(LT[0])[i] = src[i];
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (ch + 1 < NCH) {
#pragma unroll
        for (int i = 0; i < PER; ++i) stage[i] = src[(int64_t)(ch + 1) * (Gm::CHUNK / 2) + tid + i * kThreads];
      }
      if (stream_b && ch + kAhead < NCH) load_chunk(ch + kAhead);
      const double2 *La = reinterpret_cast<const double2 *>(LT[ch & 1]) + lane;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = 4 * ch + u;
        if (ch + 1 < NCH || u == 0 || kk < KK) {
#pragma unroll
          for (int p = 0; p < Gm::P; ++p) {
            const double2 a = La[(u * Gm::P + p) * 64];
            acc[2 * p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, be[kk], acc[2 * p], 0, 0, 0);
            acc[2 * p + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bo[kk], acc[2 * p + 1], 0, 0, 0);
          }
        }
      }
      if (ch + 1 < NCH) {
        if constexpr (PER > 0) {
#pragma unroll
          for (int i = 0; i < PER; ++i) reinterpret_cast<double2 *>(LT[(ch + 1) & 1])[tid + i * kThreads] = stage[i];
        } else {
          for (int i = tid; i < Gm::CHUNK / 2; i += kThreads) reinterpret_cast<double2 *>(LT[(ch + 1) & 1])[i] = src[(int64_t)(ch + 1) * (Gm::CHUNK / 2) + i];
        }
      }
      __syncthreads();
    }
  };

  gemm(reinterpret_cast<const double *>(P.T1[c]), b0, b1, true);
  if constexpr (MODE == 2) {
    double base = 0;
    const int64_t col = min(P.col0 + nc, P.col_total - 1);
    if (P.lam1[c]) { const int64_t jj = col / P.n0; base = P.k0[c] * P.lam0[c][col - jj * P.n0] + P.k1[c] * P.lam1[c][jj]; }
    else if (P.lam0[c]) base = P.k0[c] * P.lam0[c][col];
    double c0[Gm::KKP], c1[Gm::KKP];
    const double *lam_lane = P.lam_d[c]; const double kdc = P.kd[c];
#pragma unroll
    for (int p = 0; p < Gm::P; ++p) {       // D register (tile p, q) of this lane = B operand of k-step 4 p + q of the same parity group
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = 16 * p + kq + 4 * q;
        const double de = fma(kdc, lam_lane[min(m, k_last)], base), dof_ = fma(kdc, lam_lane[min(ne + m, k_last)], base);
        double re = __builtin_amdgcn_rcp(de), ro = __builtin_amdgcn_rcp(dof_);
        re = de < 1e300 ? fma(re, fma(-de, re, 1.0), re) : 0.0; ro = dof_ < 1e300 ? fma(ro, fma(-dof_, ro, 1.0), ro) : 0.0;
        c0[4 * p + q] = m < ne ? acc[2 * p][q] * re : 0.0;
        c1[4 * p + q] = ne + m < nn ? acc[2 * p + 1][q] * ro : 0.0;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    gemm(reinterpret_cast<const double *>(P.T2[c]), c0, c1, false);
  }
  if (!valid) return;
  if constexpr (MODE == 0) {                 // modes: even ones at m, odd ones behind them; slots behind the last mode get the zeros of the padded rows
#pragma unroll
    for (int p = 0; p < Gm::P; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = 16 * p + kq + 4 * q;
        if (m < ne) out_lane[(int64_t)m * out_stride] = acc[2 * p][q];
        if (ne + m < nn) out_lane[(int64_t)(ne + m) * out_stride] = acc[2 * p + 1][q];
      }
  } else {                                   // nodes: x_k = a + b, x_{n-1-k} = a - b
#pragma unroll
    for (int p = 0; p < Gm::P; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 16 * p + kq + 4 * q;
        if (k >= h) continue;
        const double a = acc[2 * p][q], b = acc[2 * p + 1][q];
        const int km = k_last - k;
        out_lane[(int64_t)k * out_stride] = km == k ? a : a + b;
        if (km != k) out_lane[(int64_t)km * out_stride] = a - b;
      }
  }
}

// ---- even / odd form for long lines (> 160 points: 2D config 2 has 673, a 128^3 Q2 box 257) ------------------------------------------------
// Same arithmetic as k_fdmu_split, but the 2 x 5 accumulator tiles cover only 80 output rows per parity: the rows are produced block by block, each block
// streaming ALL k-steps of its slice of the transform matrix through LDS while the data fragments are re-read (L2) and, for the forward direction,
// butterflied again.  Loops are runtime loops (the line length is arbitrary), the data fragments of the next chunk are requested one chunk ahead.
// MODE 0 forward, 1 backward (optionally dividing the coefficients by the eigenvalue sums on load: the last direction, whose forward / backward
// pair cannot be chained through registers at this length).
template <int MODE>
__global__ void __launch_bounds__(kThreads, 2)
k_fdmu_blk(FdmuPass P, const double *__restrict__ in, double *__restrict__ out) {
  constexpr int PP = 5, CHUNK = 4 * PP * 128, PER = CHUNK / 2 / kThreads;
  __shared__ double LT[2][CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y, j = lane & 15, kq = lane >> 4;
  const int64_t n = (int64_t)blockIdx.x * 64 + w * 16 + j;
  const bool valid = n < P.n_lines;
  const int64_t nc = valid ? n : P.n_lines - 1;
  const int64_t lb = P.SI == 1 ? nc * P.nK : line_base(P, nc);
  const int64_t in_stride = P.in_interleaved ? P.SI * P.ncomp : P.SI, out_stride = P.out_interleaved ? P.SI * P.ncomp : P.SI;
  const double *in_lane = in + (P.in_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb);
  double *out_lane = out + (P.out_interleaved ? lb * P.ncomp + c : (int64_t)c * P.comp_stride + lb);
  const int nn = P.nK, h = (nn + 1) / 2, ne = P.n_even[c], k_last = nn - 1;
  const int NCHK = P.blk_nch[c], KK = P.blk_kk[c];
  double base = 0; const double *lam_lane = nullptr; double kdc = 0;
  if (MODE == 1 && P.scale_on_load) {
    const int64_t col = min(P.col0 + nc, P.col_total - 1);
    if (P.lam1[c]) { const int64_t jj = col / P.n0; base = P.k0[c] * P.lam0[c][col - jj * P.n0] + P.k1[c] * P.lam1[c][jj]; }
    else if (P.lam0[c]) base = P.k0[c] * P.lam0[c][col];
    lam_lane = P.lam_d[c]; kdc = P.kd[c];
  }
  auto load_chunk = [&](int ch, double (&b0)[4], double (&b1)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = 4 * (4 * ch + u) + kq;
      if (MODE == 1) {
        const int ie = min(k, k_last), io = min(ne + k, k_last);
        double ve = in_lane[(int64_t)ie * in_stride], vo = in_lane[(int64_t)io * in_stride];
        if (lam_lane) {
          const double de = fma(kdc, lam_lane[ie], base), dd = fma(kdc, lam_lane[io], base);
          double re = __builtin_amdgcn_rcp(de), ro = __builtin_amdgcn_rcp(dd);
          re = de < 1e300 ? fma(re, fma(-de, re, 1.0), re) : 0.0; ro = dd < 1e300 ? fma(ro, fma(-dd, ro, 1.0), ro) : 0.0;
          ve *= re; vo *= ro;
        }
        b0[u] = ve; b1[u] = vo;
      } else {
        const int kc = min(k, h - 1), km = k_last - kc;
        const double lo = in_lane[(int64_t)kc * in_stride], hi = in_lane[(int64_t)km * in_stride];
        b0[u] = km == kc ? lo : lo + hi; b1[u] = lo - hi;
      }
    }
  };
  // one row block per workgroup (grid z): a 2D mesh has few lines (673 per component at config 2), the row blocks supply the missing parallelism
  for (int mb = blockIdx.z; mb < P.blk_mb[c]; mb += gridDim.z) {
    v4d acc[2 * PP];
#pragma unroll
    for (int t = 0; t < 2 * PP; ++t) acc[t] = v4d{0, 0, 0, 0};
    const double2 *src = reinterpret_cast<const double2 *>(reinterpret_cast<const double *>(P.T1[c]) + (int64_t)mb * NCHK * CHUNK);
    double2 stage[PER];
    double b0[4], b1[4], n0[4], n1[4];
    __syncthreads();                                        // the previous row block has finished with both LDS buffers
#pragma unroll
    for (int i = 0; i < PER; ++i) reinterpret_cast<double2 *>(LT[0])[tid + i * kThreads] = src[tid + i * kThreads];
    load_chunk(0, b0, b1);
    __syncthreads();
    for (int ch = 0; ch < NCHK; ++ch) {
      const bool more = ch + 1 < NCHK;
      if (more) {
#pragma unroll
        for (int i = 0; i < PER; ++i) stage[i] = src[(int64_t)(ch + 1) * (CHUNK / 2) + tid + i * kThreads];
        load_chunk(ch + 1, n0, n1);
      }
      const double2 *La = reinterpret_cast<const double2 *>(LT[ch & 1]) + lane;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (4 * ch + u < KK) {
#pragma unroll
          for (int p = 0; p < PP; ++p) {
            const double2 a = La[(u * PP + p) * 64];
            acc[2 * p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b0[u], acc[2 * p], 0, 0, 0);
            acc[2 * p + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b1[u], acc[2 * p + 1], 0, 0, 0);
          }
        }
      }
      if (more) {
#pragma unroll
        for (int i = 0; i < PER; ++i) reinterpret_cast<double2 *>(LT[(ch + 1) & 1])[tid + i * kThreads] = stage[i];
#pragma unroll
        for (int u = 0; u < 4; ++u) { b0[u] = n0[u]; b1[u] = n1[u]; }
      }
      __syncthreads();
    }
    if (valid) {
#pragma unroll
      for (int p = 0; p < PP; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 16 * (PP * mb + p) + kq + 4 * q;
          if (MODE == 0) {
            if (r < ne) out_lane[(int64_t)r * out_stride] = acc[2 * p][q];
            if (ne + r < nn) out_lane[(int64_t)(ne + r) * out_stride] = acc[2 * p + 1][q];
          } else if (r < h) {
            const double a = acc[2 * p][q], b = acc[2 * p + 1][q];
            const int km = k_last - r;
            out_lane[(int64_t)r * out_stride] = km == r ? a : a + b;
            if (km != r) out_lane[(int64_t)km * out_stride] = a - b;
          }
        }
    }
  }
}

inline int split_nch(int nK) { const int need = ((nK + 1) / 2 + 15) / 16; for (int v : {1, 2, 3, 4, 5}) if (need <= v) return v; return 0; }

void launch_split(hipStream_t s, const FdmuPass &P, const double *in, double *out) {
  const dim3 grid((unsigned)((P.n_lines + 63) / 64), (unsigned)P.ncomp);
  if (P.blk) {
    if (P.fused) throw Error("launch_split: the blocked form runs the last direction as two passes");
    int mbz = 1; for (int c = 0; c < P.ncomp; ++c) mbz = std::max(mbz, P.blk_mb[c]);
    const dim3 gridz(grid.x, grid.y, (unsigned)mbz);
    if (P.split_dir == 0) hipLaunchKernelGGL((k_fdmu_blk<0>), gridz, dim3(kThreads), 0, s, P, in, out);
    else hipLaunchKernelGGL((k_fdmu_blk<1>), gridz, dim3(kThreads), 0, s, P, in, out);
    return;
  }
  const int mode = P.fused ? 2 : P.split_dir;
  switch (split_nch(P.nK) * 4 + mode) {
#define PORO_SPLIT_CASE(N) case 4 * N: hipLaunchKernelGGL((k_fdmu_split<N, 0>), grid, dim3(kThreads), 0, s, P, in, out); break; \
                           case 4 * N + 1: hipLaunchKernelGGL((k_fdmu_split<N, 1>), grid, dim3(kThreads), 0, s, P, in, out); break; \
                           case 4 * N + 2: hipLaunchKernelGGL((k_fdmu_split<N, 2>), grid, dim3(kThreads), 0, s, P, in, out); break;
    PORO_SPLIT_CASE(1) PORO_SPLIT_CASE(2) PORO_SPLIT_CASE(3) PORO_SPLIT_CASE(4) PORO_SPLIT_CASE(5)
#undef PORO_SPLIT_CASE
    default: throw Error("launch_split: line too long");
  }
}

inline int reg_nch(int nK) { const int need = (nK + 15) / 16; for (int v : {1, 2, 3, 5, 7, 10}) if (need <= v) return v; return 0; }

void launch_reg(hipStream_t s, const FdmuPass &P, const double *in, double *out) {
  const dim3 grid((unsigned)((P.n_lines + 63) / 64), (unsigned)P.ncomp);
  const int mode = P.fused ? 1 : (P.SI == 1 && !std::getenv("PORO_FDMU_NO_SWAP")) ? 2 : 0;
  switch (reg_nch(P.nK) * 4 + mode) {
#define PORO_REG_CASE(N) case 4 * N: hipLaunchKernelGGL((k_fdmu_reg<N, 0>), grid, dim3(kThreads), 0, s, P, in, out); break; \
                         case 4 * N + 1: hipLaunchKernelGGL((k_fdmu_reg<N, 1>), grid, dim3(kThreads), 0, s, P, in, out); break; \
                         case 4 * N + 2: hipLaunchKernelGGL((k_fdmu_reg<N, 2>), grid, dim3(kThreads), 0, s, P, in, out); break;
    PORO_REG_CASE(1) PORO_REG_CASE(2) PORO_REG_CASE(3) PORO_REG_CASE(5) PORO_REG_CASE(7) PORO_REG_CASE(10)
#undef PORO_REG_CASE
    default: throw Error("launch_reg: line too long");
  }
}

template <class TC, class TIn, class TOut>
void launch_pass(hipStream_t s, const FdmuPass &P, const TIn *in, TOut *out) {
  if constexpr (std::is_same<TC, double>::value && std::is_same<TIn, double>::value && std::is_same<TOut, double>::value) {
    if (P.split) { launch_split(s, P, in, out); return; }
    if (P.reg_form) { launch_reg(s, P, in, out); return; }
  }
  const int rows = std::max(P.KK * 4, P.MT * 16);
  const size_t lds = sizeof(TC) * (size_t)(P.x_layout ? kNT * P.ld_line : rows * kLdK);
  const dim3 grid((unsigned)((P.n_lines + kNT - 1) / kNT), (unsigned)P.ncomp);
  const int mth = (P.MT + 1) / 2;
#define PORO_FDMU_CASE(M)                                                                                                          \
  { static bool set_##M[64] = {false}; int dev = 0; (void)hipGetDevice(&dev);                                                    \
    if (dev < 64 && !set_##M[dev]) { PORO_HIP(hipFuncSetAttribute((const void *)k_fdmu_pass<TC, TIn, TOut, M>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); set_##M[dev] = true; } \
    hipLaunchKernelGGL((k_fdmu_pass<TC, TIn, TOut, M>), grid, dim3(kThreads), lds, s, P, in, out); }
  if (mth <= 1) PORO_FDMU_CASE(1)
  else if (mth <= 2) PORO_FDMU_CASE(2)
  else if (mth <= 3) PORO_FDMU_CASE(3)
  else if (mth <= 5) PORO_FDMU_CASE(5)
  else if (mth <= 7) PORO_FDMU_CASE(7)
  else if (mth <= 10) PORO_FDMU_CASE(10)
  else throw Error("fast diagonalisation of the displacement system: more than 320 nodes per grid line");
#undef PORO_FDMU_CASE
}

// ---- host: the tables of one line (fdm_tables.hpp) in the fragment orders of the kernels above ------------------------------------------------
// full-length forms, S^T forward and S backward.  Register form (k_fdmu_reg): chunked order [chunk][k-step u][tile pair p][lane][2] with tile 2p + e of the one
// matrix in entry e; LDS form (k_fdmu_pass): [MT][KK][64] in the precision of the transforms
void upload_full(FdmuDir &D, const LineTables &T, bool single) {
  const int nn = T.n; const std::vector<double> &S = T.S;
  auto fwd = [&](int r, int c) { return S[(size_t)c * nn + r]; };
  auto bwd = [&](int r, int c) { return S[(size_t)r * nn + c]; };
  if (D.reg_form) {
    const int nch = reg_nch(nn), mtp = (nch + 1) / 2;
    auto tile = [](int, int p, int e) { return 2 * p + e; };
    D.fwd.upload(pack_paired_chunks(1, nch, mtp, tile, [&](int r, int c, int) { return r < nn && c < nn ? fwd(r, c) : 0.0; }));
    D.bwd.upload(pack_paired_chunks(1, nch, mtp, tile, [&](int r, int c, int) { return r < nn && c < nn ? bwd(r, c) : 0.0; }));
  } else {
    const int MT = (nn + 15) / 16, KK = (nn + 3) / 4;
    if (single) {       // (64 floats per fragment: the buffers of doubles hold them exactly)
      const std::vector<float> f = pack_fragments<float>(MT, KK, nn, nn, fwd), b = pack_fragments<float>(MT, KK, nn, nn, bwd);
      D.fwd.upload(reinterpret_cast<const double *>(f.data()), f.size() / 2); D.bwd.upload(reinterpret_cast<const double *>(b.data()), b.size() / 2);
    }
    else { D.fwd.upload(pack_fragments<double>(MT, KK, nn, nn, fwd)); D.bwd.upload(pack_fragments<double>(MT, KK, nn, nn, bwd)); }
  }
  D.lam.upload(T.lam);
}
// even / odd form: the half-size matrices of the two parity groups side by side (entry 0 = even product, 1 = odd product).  Forward: rows = modes of the group,
// columns = lower-half nodes; backward: rows = lower-half nodes, columns = modes.  k_fdmu_split: [chunk][k-step u][tile p][lane][2]; lines too long for it:
// the blocked order of k_fdmu_blk, [row block][chunk][k-step u][tile p][lane][2] with 80 rows per parity and block
void upload_split(FdmuDir &D, const LineTables &T) {
  if (!T.parity) throw Error("fdmu_upload_dir: the even / odd form needs tables whose modes are all even or odd");      // (then a parity group fits the half line)
  const int nn = T.n, h = (nn + 1) / 2, nch = split_nch(nn), ne = (int)T.even.size(), no = (int)T.odd.size();
  const std::vector<double> &S = T.S; const std::vector<int> *const grp[2] = {&T.even, &T.odd};
  auto fwd = [&](int r, int c, int e) { const std::vector<int> &g = *grp[e]; return r < (int)g.size() && c < h ? S[(size_t)c * nn + g[r]] : 0.0; };
  auto bwd = [&](int r, int c, int e) { const std::vector<int> &g = *grp[e]; return r < h && c < (int)g.size() ? S[(size_t)r * nn + g[c]] : 0.0; };
  if (nch) {
    auto tile = [](int, int p, int) { return p; };
    D.fwd.upload(pack_paired_chunks(1, nch, nch, tile, fwd)); D.bwd.upload(pack_paired_chunks(1, nch, nch, tile, bwd));
  } else {
    constexpr int PP = 5;
    auto tile = [](int b, int p, int) { return PP * b + p; };
    for (int w = 0; w < 2; ++w) {       // forward, backward
      const int rows = w == 0 ? std::max(ne, no) : h, cols = w == 0 ? h : std::max(ne, no);
      const int kk = (cols + 3) / 4, nchk = (kk + 3) / 4, mb = (rows + 16 * PP - 1) / (16 * PP);
      if (w == 0) D.fwd.upload(pack_paired_chunks(mb, nchk, PP, tile, fwd)); else D.bwd.upload(pack_paired_chunks(mb, nchk, PP, tile, bwd));
      D.blk_kk[w] = kk; D.blk_nch[w] = nchk; D.blk_mb[w] = mb;
    }
  }
  std::vector<double> lp(nn, std::numeric_limits<double>::infinity());      // mode order along the line: the even modes first, then the odd ones
  for (int i = 0; i < ne; ++i) lp[i] = T.lam[T.even[i]];
  for (int i = 0; i < no; ++i) lp[ne + i] = T.lam[T.odd[i]];
  D.lam.upload(lp); D.n_even = ne; D.split = true; D.blk = !nch;
}
}  // namespace

void fdmu_upload_dir(FdmuDir &D, const LineTables &T, bool single, bool allow_split) {
  const int nn = T.n;
  D.n = nn; D.split = false; D.blk = false; D.n_even = 0; D.reg_form = !single && reg_nch(nn) > 0 && !std::getenv("PORO_FDMU_LDS_FORM");
  if (!single && allow_split && !std::getenv("PORO_FDMU_LDS_FORM") && !std::getenv("PORO_FDMU_NO_SPLIT")) { upload_split(D, T); return; }
  if (nn > 320) throw Error("fast diagonalisation of the displacement system: a line of more than 320 points needs the even / odd form (the same Dirichlet condition at both ends of every direction)");
  upload_full(D, T, single);
}

// z = blockdiag(A_cc)^-1 g.  g, z: node-interleaved vectors of the local grid nn[0] x nn[1] (x nn[2]); t1, t2: planar scratch of the same size.
// z_lines != null (partitioned run): the last-direction pass works on whole global lines of this rank's column group, which the caller
// gathers / scatters around it (see ctx.hip); then only the passes of the leading directions run here (stage 0: forward, 1: backward).
// fills the pass descriptor of direction d of a grid nn[0] x nn[1] (x nn[2]) from the per-(component, direction) data `dirs[c]`
static void fill_dir(FdmuPass &P, const FdmuDir *const dirs[3], int dim, bool fwd) {
  P.reg_form = dirs[0]->reg_form ? 1 : 0;
  P.split = 1; P.split_dir = fwd ? 0 : 1; P.blk = 1;
  for (int c = 0; c < dim; ++c) { P.split = P.split && dirs[c]->split; P.blk = P.blk && dirs[c]->blk; P.n_even[c] = dirs[c]->n_even; }
  if (!P.split) P.blk = 0;
  if (P.blk) { const int w = fwd ? 0 : 1; for (int c = 0; c < dim; ++c) { P.blk_kk[c] = dirs[c]->blk_kk[w]; P.blk_nch[c] = dirs[c]->blk_nch[w]; P.blk_mb[c] = dirs[c]->blk_mb[w]; } }
}
template <class TC> static void fdmu_apply_t(hipStream_t s, const FdmU &F, const double *g, double *z, void *t1v, void *t2v, int stage) {
  TC *t1 = reinterpret_cast<TC *>(t1v), *t2 = reinterpret_cast<TC *>(t2v);
  const int dim = F.dim; const int64_t nx = F.nn[0], ny = F.nn[1], nz = dim == 3 ? F.nn[2] : 1, nnode = nx * ny * nz;
  auto pass = [&](int d, bool fwd, bool fused) {
    FdmuPass P{};
    P.nK = F.nn[d]; P.MT = (P.nK + 15) / 16; P.KK = (P.nK + 3) / 4;
    P.SI = d == 0 ? 1 : d == 1 ? nx : nx * ny; P.n_lines = nnode / P.nK; P.comp_stride = nnode; P.ncomp = dim;
    P.x_layout = d == 0 ? 1 : 0; P.ld_line = std::max(P.KK * 4, P.MT * 16) + 2;
    P.fused = fused ? 1 : 0; P.n0 = (int)nx; P.col0 = 0; P.col_total = P.n_lines;
    const FdmuDir *dirs[3] = {&F.dir[0][d], &F.dir[dim > 1 ? 1 : 0][d], &F.dir[dim > 2 ? 2 : 0][d]};
    fill_dir(P, dirs, dim, fwd);
    for (int c = 0; c < dim; ++c) {
      const FdmuDir &D = F.dir[c][d];
      P.T1[c] = (fwd || fused) ? (const void *)D.fwd.p : (const void *)D.bwd.p; P.T2[c] = D.bwd.p;
      P.lam_d[c] = D.lam.p; P.kd[c] = F.coef[c][d];
      P.lam0[c] = F.dir[c][0].lam.p; P.k0[c] = F.coef[c][0];
      P.lam1[c] = dim == 3 ? F.dir[c][1].lam.p : nullptr; P.k1[c] = dim == 3 ? F.coef[c][1] : 0.0;
    }
    return P;
  };
  const int last = dim - 1;
  if (stage == 0 || stage == 2) {
    FdmuPass P = pass(0, true, false); P.in_interleaved = 1;
    launch_pass<TC, double, TC>(s, P, g, t1);                                    // x forward: g (interleaved) -> t1 (planar)
    if (dim == 3) { P = pass(1, true, false); launch_pass<TC, TC, TC>(s, P, t1, t2); }   // y forward: t1 -> t2
  }
  TC *cur = dim == 3 ? t2 : t1, *other = dim == 3 ? t1 : t2;                    // where the data are after the leading directions
  if (stage == 2) {                                                               // single rank: last direction forward + scale + backward
    FdmuPass P = pass(last, true, true);
    if (P.blk) {                                                                  // long lines: two passes, the scaling rides on the backward pass's loads
      P.fused = 0; launch_pass<TC, TC, TC>(s, P, cur, other);
      FdmuPass Q = pass(last, false, false); Q.scale_on_load = 1; launch_pass<TC, TC, TC>(s, Q, other, cur);
    } else { launch_pass<TC, TC, TC>(s, P, cur, other); std::swap(cur, other); }
  }
  if (stage == 1 || stage == 2) {
    // stage 1 (partitioned): the caller scattered the result of the last direction back into `cur`
    if (dim == 3) {
      FdmuPass P = pass(1, false, false);
      launch_pass<TC, TC, TC>(s, P, cur, other); std::swap(cur, other);
    }
    FdmuPass P = pass(0, false, false); P.out_interleaved = 1;
    launch_pass<TC, TC, double>(s, P, cur, z);
  }
}
// copy a (component, planes, columns) window between a planar grid array [c][grid_planes][grid_stride] and a dense, zero-padded block
// [c][n_planes_pad][C] (to_block) or back: the pieces of the all-to-all that hands whole lines of the partitioned direction to a rank
__global__ void k_fdmu_window(double *dst, const double *src, int to_block, int ncomp, int n_planes, int n_planes_pad, int64_t C, int64_t ncols_valid,
                              int64_t grid_stride, int64_t grid_planes, int64_t grid_col0, int64_t grid_plane0) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)ncomp * n_planes_pad * C) return;
  const int64_t cc = idx % C, rest = idx / C, k = rest % n_planes_pad, comp = rest / n_planes_pad;
  const bool valid = k < n_planes && cc < ncols_valid;
  const int64_t g = (comp * grid_planes + grid_plane0 + k) * grid_stride + grid_col0 + cc;
  if (to_block) dst[idx] = valid ? src[g] : 0.0;
  else if (valid) dst[g] = src[idx];
}
void fdmu_window(hipStream_t s, double *dst, const double *src, bool to_block, int ncomp, int n_planes, int n_planes_pad, int64_t C, int64_t ncols_valid,
                 int64_t grid_stride, int64_t grid_planes, int64_t grid_col0, int64_t grid_plane0) {
  const int64_t n = (int64_t)ncomp * n_planes_pad * C;
  if (n) hipLaunchKernelGGL(k_fdmu_window, (unsigned)((n + 255) / 256), 256, 0, s, dst, src, to_block ? 1 : 0, ncomp, n_planes, n_planes_pad, C, ncols_valid, grid_stride, grid_planes, grid_col0, grid_plane0);
}

void fdmu_apply(hipStream_t s, const FdmU &F, const double *g, double *z, void *t1, void *t2, int stage) {
  if (F.single) fdmu_apply_t<float>(s, F, g, z, t1, t2, stage); else fdmu_apply_t<double>(s, F, g, z, t1, t2, stage);
}

// the fused last-direction pass on a column-distributed array [component][global line point][C local columns] (partitioned runs)
template <class TC> static void fdmu_lines_t(hipStream_t s, const FdmU &F, const FdmuDir *last_dir /*[dim]*/, int64_t C, int64_t col0, int64_t ncol_valid, void *in_v, void *out_v) {
  const int dim = F.dim, last = dim - 1;
  auto pass = [&](bool fwd, bool fused) {
    FdmuPass P{};
    P.nK = last_dir[0].n; P.MT = (P.nK + 15) / 16; P.KK = (P.nK + 3) / 4;
    P.SI = C; P.n_lines = C; P.comp_stride = (int64_t)P.nK * C; P.ncomp = dim; P.x_layout = 0; P.ld_line = 0;
    P.fused = fused ? 1 : 0; P.n0 = F.nn[0]; P.col0 = col0; P.col_total = col0 + ncol_valid;   // padding columns hold zeros and stay zero
    const FdmuDir *dirs[3] = {&last_dir[0], &last_dir[dim > 1 ? 1 : 0], &last_dir[dim > 2 ? 2 : 0]};
    fill_dir(P, dirs, dim, fwd);
    for (int c = 0; c < dim; ++c) {
      P.T1[c] = (fwd || fused) ? last_dir[c].fwd.p : last_dir[c].bwd.p; P.T2[c] = last_dir[c].bwd.p; P.lam_d[c] = last_dir[c].lam.p; P.kd[c] = F.coef[c][last];
      P.lam0[c] = F.dir[c][0].lam.p; P.k0[c] = F.coef[c][0];
      P.lam1[c] = dim == 3 ? F.dir[c][1].lam.p : nullptr; P.k1[c] = dim == 3 ? F.coef[c][1] : 0.0;
    }
    return P;
  };
  TC *in = reinterpret_cast<TC *>(in_v), *out = reinterpret_cast<TC *>(out_v);
  FdmuPass P = pass(true, true);
  if (P.blk) {
    P.fused = 0; launch_pass<TC, TC, TC>(s, P, in, out);
    FdmuPass Q = pass(false, false); Q.scale_on_load = 1; launch_pass<TC, TC, TC>(s, Q, out, in);
    PORO_HIP(hipMemcpyAsync(out, in, sizeof(TC) * (size_t)dim * P.nK * C, hipMemcpyDeviceToDevice, s));
  } else launch_pass<TC, TC, TC>(s, P, in, out);
}
void fdmu_lines(hipStream_t s, const FdmU &F, const FdmuDir *last_dir, int64_t C, int64_t col0, int64_t ncol_valid, void *in, void *out) {
  if (F.single) fdmu_lines_t<float>(s, F, last_dir, C, col0, ncol_valid, in, out); else fdmu_lines_t<double>(s, F, last_dir, C, col0, ncol_valid, in, out);
}

}  // namespace poro
