// Prioritised mixture sampling over the on-HBM replay ring and the per-sequence priorities of a learner step (gfx950).
//
// priority[i] (fp32, one per ring slot; 0 = unfilled) is P = (p_raw + eps)^alpha, p_raw = eta·max_t|A_t| +
// (1 − eta)·mean_t|A_t| over the sequence's valid rows, A the un-normalised in-step V-trace advantages of the step
// that last trained on it (scan.hip vtrace_step_kernel). Each of the B draws of a minibatch takes two uniforms
// (u0, u1) in [0, 1) of 24 random bits from a counter-based hash (seed, draw counter, draw, which — the idiom of
// actor.hip): u0 < recent_frac → uniform over the newest m slots, idx = (cursor − 1 − min(m − 1, ⌊u1·m⌋)) mod capacity;
// else the smallest idx whose inclusive prefix sum of P exceeds u1·ΣP. All sums in double, in a fixed order.
//
//   1. priority_block_sums_kernel — one workgroup per 4096-slot block: every thread sums its 16 consecutive slots in
//      slot order, the 256 thread sums are folded by a butterfly over the wave and over the 4 waves in LDS (a fixed
//      tree). Writes the block's double sum and fp32 maximum.
//   2. replay_sample_kernel — ONE workgroup. Thread 0 scans the ≤ 256 block sums in LDS; then one wave per draw:
//      binary search of the block, every lane sums its 64 consecutive slots of that block, a wave scan of the lane
//      sums finds the lane and that lane walks its slots. If rounding between the block sums' tree and this scan
//      leaves no crossing, the draw takes the block's last slot with P > 0. Writes idx into the caller's buffer (the
//      captured step's static index buffer), the maximum priority, the next draw counter, the statistics
//      {newest-window draws, Σ (current version − version[idx]), Σ P[idx], max P} and optionally the uniforms it used.
//      With `w_out` also every draw's importance-sampling weight: q(idx) = f·[idx in the newest window]/m +
//      (1 − f)·P[idx]/ΣP is the slot's probability under the whole mixture (whichever branch drew it; ΣP ≤ 0:
//      [in window]/m), w = (size·q)^(−beta) in double (q = 0, reachable only through the clamped fall-backs: w = 1,
//      counted), w_out[d] = float(w / max_d w). The maximum goes over the wave partials in LDS, then every wave forms
//      its draws' weights again and divides; statistics {Σ w_out, min w_out, draws with q = 0} behind the first four.
//   3. seq_priority_kernel — one workgroup per sequence over the time-major rows r = t·B + b of the step's advantages:
//      tree reduction of max / sum / count over the valid rows → out[b] = P, out[B + b] = non-finite flag.
//   4. priority_scatter_kernel — priority[idx[b]] = P[b] (duplicates carry equal values) and the non-finite counter.
//
// No atomics, no inline assembly: every cross-thread value goes through shuffles or LDS inside one workgroup, every
// cross-kernel value through stream order.
#include "common.h"

namespace {

constexpr int kT = 256;
constexpr int kBlock = 4096;                 // slots per block sum
constexpr int kPer = kBlock / kT;            // 16 consecutive slots per thread in kernel 1
constexpr int kMaxBlocks = 256;              // capacity ≤ 2^20
constexpr int kLane = kBlock / dca::kWave;   // 64 consecutive slots per lane in kernel 2
constexpr int kChunk = 16;                   // ... read 16 at a time
constexpr int kTS = 512;                     // sampler workgroup: 8 waves
constexpr int kWS = kTS / dca::kWave;

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// uniform in [0, 1) with 24 random bits
__device__ __forceinline__ float uniform24(unsigned long long seed, unsigned long long ctr, int draw, int which) {
  const unsigned long long h = mix64(seed ^ mix64(ctr ^ mix64(((unsigned long long)draw << 1) | (unsigned)which)));
  return (float)(h >> 40) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ double shfl_xor_d(double v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ double shfl_up_d(double v, int o) { return __shfl_up(v, o, 64); }

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// `n` (≤ N) consecutive slots starting at p[base] into v[0..N) (zeros past `cap`); float4 loads when whole and aligned
template <int N>
__device__ __forceinline__ void load_run(const float* __restrict__ p, long long base, long long cap, bool vec,
                                         float (&v)[N]) {
  if (vec && base + N <= cap) {
#pragma unroll
    for (int j = 0; j < N; j += 4) {
      const float4 q = *reinterpret_cast<const float4*>(p + base + j);
      v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (base + j < cap) ? p[base + j] : 0.f;
  }
}

// un-normalised importance-sampling weight of slot `idx` under the mixture (see the header); `zero` ← (q = 0).
// No contraction: the float64 oracle (ops/replay.py importance_weights_reference) rounds every operation.
__device__ __forceinline__ double is_weight_raw(const float* __restrict__ pri, long long idx, int capacity, int size,
                                                int cursor, int m, double f, double T, double beta, bool& zero) {
#pragma clang fp contract(off)
  const long long back = (((long long)cursor - 1 - idx) % capacity + capacity) % capacity;
  const double win = back < (long long)m ? 1.0 / (double)m : 0.0;
  const double q = T > 0.0 ? f * win + (1.0 - f) * ((double)pri[idx] / T) : win;
  zero = !(q > 0.0);
  return zero ? 1.0 : pow((double)size * q, -beta);
}

__global__ __launch_bounds__(kT) void priority_block_sums_kernel(const float* __restrict__ pri, int capacity,
                                                                 double* __restrict__ bsum, float* __restrict__ bmax) {
  const long long base = (long long)blockIdx.x * kBlock + (long long)threadIdx.x * kPer;
  float v[kPer];
  load_run<kPer>(pri, base, capacity, aligned16(pri), v);
  double s = 0.0;
  float mx = 0.f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    s += (double)v[j];
    mx = fmaxf(mx, v[j]);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += shfl_xor_d(s, o);
  mx = dca::wave_max(mx);
  __shared__ double ws[kT / 64];
  __shared__ float wm[kT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    ws[w] = s;
    wm[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    bmax[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  }
}

__global__ __launch_bounds__(kTS) void replay_sample_kernel(
    const float* __restrict__ pri, const long long* __restrict__ version, const double* __restrict__ bsum,
    const float* __restrict__ bmax, int nblk, int capacity, int size, int cursor, int m, float recent_frac,
    long long cur_version, unsigned long long seed, long long* __restrict__ ctr, long long* __restrict__ idx_out,
    int B, float* __restrict__ pmax_out, double* __restrict__ stats, float* __restrict__ u_out, double beta,
    float* __restrict__ w_out) {
  __shared__ double pre[kMaxBlocks];          // inclusive prefix sums of the block sums
  __shared__ float smax[kMaxBlocks];
  __shared__ double red[3][kWS];
  __shared__ double wred[2][kWS];             // importance weights: wave maxima / q = 0 counts, then sums / minima
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < nblk) {
    pre[tid] = bsum[tid];
    smax[tid] = bmax[tid];
  }
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    float mx = 0.f;
    for (int k = 0; k < nblk; ++k) {
      run += pre[k];
      pre[k] = run;
      mx = fmaxf(mx, smax[k]);
    }
    *pmax_out = mx;
    stats[3] = (double)mx;
  }
  __syncthreads();
  const unsigned long long c = (unsigned long long)*ctr;
  const double T = pre[nblk - 1];
  const bool vec = aligned16(pri);
  double n_new = 0.0, age = 0.0, psum = 0.0;   // this wave's statistics (lane 0 holds them)
  double wmax = 0.0, nzero = 0.0;
  for (int d = w; d < B; d += kWS) {
    const float u0 = uniform24(seed, c, d, 0), u1 = uniform24(seed, c, d, 1);
    long long idx;
    const bool newest = u0 < recent_frac || !(T > 0.0);
    if (newest) {
      const long long r = min((long long)m - 1, (long long)floor((double)u1 * (double)m));
      idx = ((long long)cursor - 1 - r + 2LL * capacity) % capacity;
    } else {
      const double target = (double)u1 * T;
      // smallest block k with pre[k] > target (target < T = pre[nblk − 1])
      int lo = 0, hi = nblk - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] > target) hi = mid; else lo = mid + 1;
      }
      const int k = lo;
      const double t = target - (k ? pre[k - 1] : 0.0);
      const long long base = (long long)k * kBlock + (long long)lane * kLane;
      double s = 0.0;
      int lastpos = -1;
#pragma unroll 1
      for (int c4 = 0; c4 < kLane; c4 += kChunk) {     // 16 slots at a time: four float4 loads in flight per lane
        float v[kChunk];
        load_run<kChunk>(pri, base + c4, capacity, vec, v);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          s += (double)v[j];
          if (v[j] > 0.f) lastpos = lane * kLane + c4 + j;
        }
      }
      double incl = s;                          // inclusive scan of the lane sums, in lane order
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double up = shfl_up_d(incl, o);
        if (lane >= o) incl += up;
      }
      const double below = shfl_up_d(incl, 1);  // the prefix sum entering this lane
      int found = -1;
      const unsigned long long cross = __ballot(incl > t);
      const int L = cross ? __ffsll((long long)cross) - 1 : -1;
      if (lane == L) {                          // walk this lane's slots again (cache hits) from its entering prefix
        double run = lane ? below : 0.0;
#pragma unroll 1
        for (int c4 = 0; c4 < kLane && found < 0; c4 += kChunk) {
          float v[kChunk];
          load_run<kChunk>(pri, base + c4, capacity, vec, v);
#pragma unroll
          for (int j = 0; j < kChunk; ++j) {
            run += (double)v[j];
            if (found < 0 && v[j] > 0.f && run > t) found = lane * kLane + c4 + j;
          }
        }
      }
      if (L >= 0) found = __shfl(found, L, 64);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lastpos = max(lastpos, __shfl_xor(lastpos, o, 64));
      if (found < 0) found = lastpos;           // rounding left no crossing: the block's last slot with P > 0
      idx = found >= 0 ? (long long)k * kBlock + found : ((long long)cursor - 1 + capacity) % capacity;
    }
    idx = min(max(idx, 0LL), (long long)capacity - 1);
    if (lane == 0) {
      idx_out[d] = idx;
      if (u_out) {
        u_out[2 * d] = u0;
        u_out[2 * d + 1] = u1;
      }
      n_new += newest ? 1.0 : 0.0;
      age += (double)(cur_version - version[idx]);
      psum += (double)pri[idx];
      if (w_out) {
        bool zero;
        wmax = fmax(wmax, is_weight_raw(pri, idx, capacity, size, cursor, m, (double)recent_frac, T, beta, zero));
        nzero += zero ? 1.0 : 0.0;
      }
    }
  }
  if (lane == 0) {
    red[0][w] = n_new;
    red[1][w] = age;
    red[2][w] = psum;
    wred[0][w] = wmax;
    wred[1][w] = nzero;
  }
  __syncthreads();
  if (tid < 3) {
    double v = 0.0;
    for (int k = 0; k < kWS; ++k) v += red[tid][k];
    stats[tid] = v;
  }
  if (tid == 0) *ctr = (long long)(c + 1);
  if (w_out) {                                  // (a launch argument: the whole workgroup takes the branch or not)
    double mx = 0.0, nz = 0.0;
    for (int k = 0; k < kWS; ++k) {
      mx = fmax(mx, wred[0][k]);
      nz += wred[1][k];
    }
    __syncthreads();                            // every thread has read the maxima: wred is free again
    double sw = 0.0, mn = 1.0;
    if (lane == 0) {
      for (int d = w; d < B; d += kWS) {        // this wave's own draws again (its lane 0 wrote idx_out[d])
        bool zero;
        const float wn =
            (float)(is_weight_raw(pri, idx_out[d], capacity, size, cursor, m, (double)recent_frac, T, beta, zero) / mx);
        w_out[d] = wn;
        sw += (double)wn;
        mn = fmin(mn, (double)wn);
      }
      wred[0][w] = sw;
      wred[1][w] = mn;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, lo = 1.0;
      for (int k = 0; k < kWS; ++k) {
        s += wred[0][k];
        lo = fmin(lo, wred[1][k]);
      }
      stats[4] = s;
      stats[5] = lo;
      stats[6] = nz;
    }
  }
}

__global__ __launch_bounds__(kT) void seq_priority_kernel(const float* __restrict__ adv, const float* __restrict__ vt,
                                                          float* __restrict__ out, int B, int S, float eta,
                                                          float alpha, float eps) {
  const int b = blockIdx.x;
  float mx = 0.f, sum = 0.f, n = 0.f, bad = 0.f;
  for (int t = threadIdx.x; t < S; t += kT) {
    const size_t r = (size_t)t * B + b;
    if (vt[4 * r + 2] > 0.f) {
      const float a = fabsf(adv[r]);
      if (!isfinite(a)) bad = 1.f;
      else {
        mx = fmaxf(mx, a);
        sum += a;
      }
      n += 1.f;
    }
  }
  mx = dca::wave_max(mx);
  sum = dca::wave_sum(sum);
  n = dca::wave_sum(n);
  bad = dca::wave_max(bad);
  __shared__ float red[4][kT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][w] = mx;
    red[1][w] = sum;
    red[2][w] = n;
    red[3][w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float M = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    const float Sm = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float N = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    bool nf = fmaxf(fmaxf(red[3][0], red[3][1]), fmaxf(red[3][2], red[3][3])) > 0.f;
    const float p_raw = N > 0.f ? eta * M + (1.f - eta) * (Sm / N) : 0.f;
    nf = nf || !isfinite(p_raw);
    out[b] = powf((nf ? 0.f : p_raw) + eps, alpha);
    out[B + b] = nf ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(kT) void priority_scatter_kernel(float* __restrict__ pri, int capacity,
                                                              const long long* __restrict__ idx,
                                                              const float* __restrict__ pf, int B,
                                                              float* __restrict__ nonfinite) {
  float bad = 0.f;
  for (int b = threadIdx.x; b < B; b += kT) {
    const long long i = idx[b];
    if (i >= 0 && i < capacity) pri[i] = pf[b];
    bad += pf[B + b];
  }
  bad = dca::wave_sum(bad);
  __shared__ float red[kT / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) *nonfinite += (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" hipError_t dca_replay_sample(const float* pri, const long long* version, double* bsum, float* bmax,
                                        int capacity, int size, int cursor, int m, float recent_frac,
                                        long long cur_version, unsigned long long seed, long long* ctr,
                                        long long* idx_out, int B, float* pmax_out, double* stats, float* u_out,
                                        hipStream_t st, double beta, float* w_out) {
  if (capacity < 1 || capacity > kMaxBlocks * kBlock || B < 1 || size < 1 || size > capacity || m < 1 || m > size ||
      cursor < 0 || cursor >= capacity || (w_out && !(beta >= 0.0)))
    return hipErrorInvalidValue;
  const int nblk = (capacity + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(priority_block_sums_kernel, dim3(nblk), dim3(kT), 0, st, pri, capacity, bsum, bmax);
  DCA_CHECK_LAUNCH();
  hipLaunchKernelGGL(replay_sample_kernel, dim3(1), dim3(kTS), 0, st, pri, version, bsum, bmax, nblk, capacity, size,
                     cursor, m, recent_frac, cur_version, seed, ctr, idx_out, B, pmax_out, stats, u_out, beta, w_out);
  DCA_CHECK_LAUNCH();
  return hipSuccess;
}

extern "C" hipError_t dca_seq_priority(const float* adv, const float* vt, float* out, int B, int S, float eta,
                                       float alpha, float eps, hipStream_t st) {
  if (B <= 0 || S <= 0) return hipSuccess;
  hipLaunchKernelGGL(seq_priority_kernel, dim3(B), dim3(kT), 0, st, adv, vt, out, B, S, eta, alpha, eps);
  DCA_CHECK_LAUNCH();
  return hipSuccess;
}

extern "C" hipError_t dca_priority_scatter(float* pri, int capacity, const long long* idx, const float* pf, int B,
                                           float* nonfinite, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(priority_scatter_kernel, dim3(1), dim3(kT), 0, st, pri, capacity, idx, pf, B, nonfinite);
  DCA_CHECK_LAUNCH();
  return hipSuccess;
}
