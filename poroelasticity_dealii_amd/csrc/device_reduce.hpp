// Deterministic two-stage reductions shared by the streaming kernels (gfx950, wave64): 256-thread blocks, grids capped at kMaxPartials blocks so that
// the per-block partial sums fit one 8 KB slab which every consumer re-reduces in a fixed order (no float atomics, bitwise reproducible).
#pragma once
#include "common.hpp"

namespace poro {
namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t n, int per_thread = 4) {
  int64_t g = (n + (int64_t)kBlock * per_thread - 1) / ((int64_t)kBlock * per_thread);
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return (int)g;
}
inline int reduce_grid(int64_t n) {
  int64_t g = (n + 2047) / 2048;
  if (g < 1) g = 1;
  if (g > kMaxPartials) g = kMaxPartials;
  return (int)g;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
// block-wide sum in a fixed order (deterministic); result valid in thread 0
__device__ inline double block_sum(double v, double *sh /*[4]*/) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}
__device__ inline double block_max(double v, double *sh) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) r = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return r;
}
// block b writes its partial and zeroes the unused tail slots b+G, b+2G, ...
__device__ inline void store_partial(double *partials, double v) {
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = v;
    for (int t = blockIdx.x + gridDim.x; t < kMaxPartials; t += gridDim.x) partials[t] = 0.0;
  }
}

// sum of n block partials (default: the kMaxPartials slots of a capped grid) in a fixed order, broadcast to every thread of the block (identical bits in every block)
__device__ inline double sum_partials(const double *p, double *sh /*[5]*/, int n = kMaxPartials) {
  double v = 0;
  for (int i = threadIdx.x; i < n; i += kBlock) v += p[i];
  v = block_sum(v, sh);
  if (threadIdx.x == 0) sh[4] = v;
  __syncthreads();
  v = sh[4];
  __syncthreads();
  return v;
}
// the same sum of the kMaxPartials slots with the same bits, computed by ONE wave without LDS or a barrier (any block shape, every wave for itself): lane l plays
// threads l, 64 + l, 128 + l, 192 + l of sum_partials' 256-thread block in turn, and the butterfly of wave_sum leaves the same bits in every lane
// In two steps, so that a kernel can issue the loads, then others of its own, and add up when it needs the sum
constexpr int kPartialsPerLane = kMaxPartials / 64;
__device__ inline void load_partials_wave(const double *p, double (&v)[kPartialsPerLane]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int k = 0; k < kMaxPartials / kBlock; ++k) v[w * (kMaxPartials / kBlock) + k] = p[64 * w + lane + k * kBlock];
}
__device__ inline double sum_partials_wave(const double (&v)[kPartialsPerLane]) {
  double s[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    s[w] = 0;
#pragma unroll
    for (int k = 0; k < kMaxPartials / kBlock; ++k) s[w] += v[w * (kMaxPartials / kBlock) + k];
  }
  // wave_sum of the four values, step by step side by side: the four exchanges of a step are independent and go out together (one after the other, the 24 dependent
  // cross-lane exchanges cost the transform pass 8 us per launch)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    double t[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) t[w] = __shfl_xor(s[w], off, 64);
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w] += t[w];
  }
  return (s[0] + s[1]) + (s[2] + s[3]);
}
// gate of a launch inside a PCG iteration: closed once the solve has finished, or the stopping test in front of this preconditioner call held
__device__ inline bool pcg_gate_closed(const PcgScalars *gate) { return gate && (gate->done | gate->finishing | gate->stop); }
// PcgStopTest in the first kernel of a preconditioner call: nonzero (workgroup-uniform) when the iteration finishes the solve
// (in two steps like the sum: pcg_stop_load requests everything the decision reads)
struct PcgStopInputs { double gg_parts[kPartialsPerLane]; double tol; int max_iter; };
__device__ inline void pcg_stop_load(const PcgStopTest &T, PcgStopInputs &in) { load_partials_wave(T.gg_part, in.gg_parts); in.tol = T.sc->tol; in.max_iter = T.sc->max_iter; }
__device__ inline int pcg_stop_decide(const PcgStopTest &T, const PcgStopInputs &in) {
  const double gg = sum_partials_wave(in.gg_parts);
  const int stop = sqrt(gg) <= in.tol ? 1 : T.it >= in.max_iter ? 2 : 0;      // (k_fdmo_update_d's order: success first, then the cap)
  // workgroup 0 also leaves the sum itself, stop or not: the direction update of the iteration reads that word instead of adding up the same partials again
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { T.sc->gg = gg; if (stop) T.sc->stop = stop; }
  return stop;
}
__device__ inline int pcg_stop_test(const PcgStopTest &T) { PcgStopInputs in; pcg_stop_load(T, in); return pcg_stop_decide(T, in); }
// The same test shared out over the four waves of a 256-thread workgroup that has a barrier of its own to offer: thread t loads the kMaxPartials / kBlock partials that
// thread t of sum_partials' block adds (a quarter of the loads and none of the 24 dependent exchanges of the all-in-one-wave form above per wave), every wave leaves its
// wave_sum in sh[wave], and behind the caller's barrier every thread forms block_sum's (s0 + s1) + (s2 + s3) - the order of additions, hence the bits, of sum_partials.
//   pcg_stop_load_quarter  - requests the inputs (8 registers until the next step)
//   pcg_stop_post_quarter  - wave sum -> sh[wave]; the caller's barrier follows
//   pcg_stop_decide_quarters - behind that barrier: nonzero (workgroup-uniform) when the iteration finishes the solve
struct PcgStopQuarter { double part[kMaxPartials / kBlock]; double tol; int max_iter; };
__device__ inline void pcg_stop_load_quarter(const PcgStopTest &T, PcgStopQuarter &in) {
#pragma unroll
  for (int k = 0; k < kMaxPartials / kBlock; ++k) in.part[k] = T.gg_part[threadIdx.x + k * kBlock];
  in.tol = T.sc->tol; in.max_iter = T.sc->max_iter;
}
__device__ inline void pcg_stop_post_quarter(const PcgStopQuarter &in, double *sh /*[4]*/) {
  double v = 0;
#pragma unroll
  for (int k = 0; k < kMaxPartials / kBlock; ++k) v += in.part[k];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}
__device__ inline int pcg_stop_decide_quarters(const PcgStopTest &T, const PcgStopQuarter &in, const double *sh) {
  const double gg = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  const int stop = sqrt(gg) <= in.tol ? 1 : T.it >= in.max_iter ? 2 : 0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { T.sc->gg = gg; if (stop) T.sc->stop = stop; }
  return stop;
}
}  // namespace
}  // namespace poro
