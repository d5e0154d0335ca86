// Fused action heads + pointer attention + masked log-softmax + PPO/VPG loss + analytic gradients (gfx950).
//
// One wave per timestep row. Replaces, for every row, the reference's chain (policy.py:148-158, 171-180;
// optimizer.py:602-672): pointer logits q·embᵀ, four masked log-softmaxes, selection by the one-hot action,
// clipped surrogate / VPG term, per-head masked entropy and the value loss — and writes the gradient of the
// batch loss w.r.t. every head input in the same pass (no autograd graph, no masked_select, no host sync):
//
//   z   (N, ldz) f32 : [ q (128) | enum (3) | x (9) | y (9) | value (1) | pad ]  (output of ONE heads GEMM)
//   emb (N, U, 128) bf16 : unit embeddings (pointer keys); fp32 in the F32 variant (the learner's fp32 mode)
//   dz  (N, ldz) f32 : ∂L/∂z   (dq in cols 0..127, d logits, dV)  → feeds the heads GEMM backward
//   dtl (N, U)  f32  : ∂L/∂(target logits)                         → ∂L/∂emb = dtl ⊗ q (encoder backward)
//   part(nblk, 16)   : per-block partial sums of the loss terms / metrics (reduced on the host side)
//
// The batch normalisers (valid steps, selections per head) depend only on the experience, so they are computed
// before this kernel and passed in `norms`; every row's gradient is then final in one pass.
//   norms[0] = 1/n_valid  norms[1] = 1/total_selections  norms[2..5] = 1/n_sel[head] (0 if none)
//   norms[6] = Σ G_last (VPG compat value-bug term)
//
// seqw (B floats, optional): per-sequence loss weights of a prioritised replay's minibatch (importance-sampling
// weights, replay_sample.hip). Rows are time-major, so row n belongs to sequence n % B; its weight multiplies the
// row's policy, value and entropy terms and their gradients (PPO-family objectives). The normalisers and the
// diagnostic sums (part[6], [7], [8], [11]) stay unweighted. Without seqw the weight is the constant 1: the products
// are exact, the outputs bit-identical.
//
// emb is the kernel's HBM traffic (229 MB of fp32 at N = 11 200, U = 40: it ran at HBM speed loading all of it), and
// most of it cannot reach the result: only units with a target-head mask or action byte set are loaded (on the
// learner's 1v1 experience 11 % of the (row, unit) pairs, two thirds of the rows none) — see `need` below.
#include "common.h"

namespace {

constexpr int kRowsPerBlock = 4;
constexpr int kQ = 128;
constexpr int kNPart = 16;

struct Params {
  const float* z; int ldz;
  const void* emb;
  const unsigned char* act; const unsigned char* msk; int A;
  const float* adv; const float* ret; const float* logp_old; const float* nret;
  const float* norms;
  float* dz; float* dtl; float* part; float* logp_out;
  short* dz16;   // if set: ∂L/∂z written in bf16 here instead of f32 to dz (what the backward GEMMs consume)
  int N, U, algo, compat_value_bug, S_bug, B_bug;
  float clip_eps, ent_coef, vf_coef;
  const float* seqw; int B;
};

__device__ __forceinline__ void put_dz(const Params& P, size_t i, float v) {
  if (P.dz16) P.dz16[i] = dca::f2bf(v);
  else P.dz[i] = v;
}

// exp / log: the hardware approximations (v_exp_f32 / v_log_f32 based) by default; libm's correctly-rounded-class
// expf / logf in the fp32-exact learner (PRECISE), whose ∂L/∂z feeds gradients summed over 11 200 rows
template <bool PRECISE>
__device__ __forceinline__ float xexp(float x) { return PRECISE ? expf(x) : __expf(x); }
template <bool PRECISE>
__device__ __forceinline__ float xlog(float x) { return PRECISE ? logf(x) : __logf(x); }

// masked log-softmax of one head held one entry per lane (lane < W); returns logp for the lane's entry.
template <bool PRECISE>
__device__ __forceinline__ void head_lsm(float logit, bool m, int lane, int W, float& logp, float& p) {
  const bool in = lane < W;
  const float v = (in && m) ? logit : -INFINITY;
  float mx = dca::wave_max(v);
  const bool any = mx > -INFINITY;
  if (!any) mx = 0.f;
  const float e = (in && m) ? xexp<PRECISE>(logit - mx) : 0.f;
  float s = dca::wave_sum(e);
  if (!(s > 0.f)) s = 1.f;
  logp = logit - mx - xlog<PRECISE>(s);
  // PRECISE: p = e / s (each entry's own rounding) instead of exp(logp), which carries the rounding of log(s) into
  // every entry of the row alike — a row-coherent error that the pointer head's ∂q sums (Σ_u ∂t_u · E1_u over 64
  // units, then over 11 200 rows that cancel ≈20×) turned into 1e-5 on its bias gradient (scripts/diag_5v5_head.py)
  p = (in && m) ? (PRECISE ? e / s : xexp<PRECISE>(logp)) : 0.f;
}

template <bool F32, bool PRECISE>
__global__ __launch_bounds__(256) void heads_loss_kernel(Params P) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int n = blockIdx.x * kRowsPerBlock + wv;
  __shared__ float s_tl[kRowsPerBlock][64];
  __shared__ float s_dtl[kRowsPerBlock][64];
  __shared__ float s_part[kRowsPerBlock][kNPart];
  __shared__ float s_zl[kRowsPerBlock][32];
  __shared__ unsigned char s_act[kRowsPerBlock][128];
  __shared__ unsigned char s_msk[kRowsPerBlock][128];
  float acc[kNPart];
#pragma unroll
  for (int i = 0; i < kNPart; ++i) acc[i] = 0.f;

  if (n < P.N) {
    const int U = P.U;
    const float* zr = P.z + (size_t)n * P.ldz;
    // ---- every global load of the row first, addresses clamped in range (a conditional load per element made the
    //      compiler wait out each one before issuing the next: ≈20 serialised round trips per row)
    const int ks = lane & 15, ug = lane >> 4;
    float q8[8];
    {
      const float4 a = *reinterpret_cast<const float4*>(zr + 8 * ks);
      const float4 b = *reinterpret_cast<const float4*>(zr + 8 * ks + 4);
      q8[0] = a.x; q8[1] = a.y; q8[2] = a.z; q8[3] = a.w; q8[4] = b.x; q8[5] = b.y; q8[6] = b.z; q8[7] = b.w;
    }
    const float zl = zr[kQ + min(lane, 21)];                 // enum | x | y logits and the value
    const float A_n = P.adv[n], R_n = P.ret[n], lpo_n = P.logp_old[n], nret_n = P.nret[n];
    // the sequence's loss weight: one value per wave (n is wave-uniform), so it lives in a scalar register
    const float w_n = P.seqw ? P.seqw[__builtin_amdgcn_readfirstlane(n) % P.B] : 1.f;
    float nm[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) nm[i] = P.norms[i];
    const unsigned char* ar = P.act + (size_t)n * P.A;
    const unsigned char* mr = P.msk + (size_t)n * P.A;
    const unsigned char a0 = ar[min(lane, P.A - 1)], a1 = ar[min(lane + 64, P.A - 1)];
    const unsigned char m0 = mr[min(lane, P.A - 1)], m1 = mr[min(lane + 64, P.A - 1)];
    constexpr int kMaxIt = 16;   // U ≤ 64
    // Units whose embedding can reach the result: a unit enters only through its pointer logit and through
    // ∂q = Σ ∂tl[u]·emb[u], and with its target-head mask byte and action byte both 0 it has p = 0, ∂tl = ±0 and an
    // a·logp term of 0 × finite. The action bit is part of `need`, so data with an action outside the mask still reads
    // its embedding. A row without needed units loads no embedding at all (wave-uniform branch, e8 = 0); elsewhere a
    // lane whose unit is not needed loads the row's FIRST NEEDED unit instead — lines its neighbours fetch anyway —
    // so the loads stay unconditional and all in flight. Unneeded units then contribute ±0 to accumulators that start
    // at +0: dz, dtl, part and logp are bit-identical to loading everything (tests/test_heads_loss_sparse.py).
    const int un = min(lane, U - 1);
    const unsigned long long need = __ballot(lane < U && (mr[21 + un] | ar[21 + un]) != 0);
    const int ufirst = need ? __ffsll((long long)need) - 1 : 0;
    // the row's unit embeddings, 8 features per lane and 4 units per wave-instruction, all loads issued up front
    float e8[kMaxIt][8];
    const int nit = (U + 3) >> 2;
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
#pragma unroll
      for (int j = 0; j < 8; ++j) e8[it][j] = 0.f;
    }
    if (need != 0) {
#pragma unroll
      for (int it = 0; it < kMaxIt; ++it)
        if (it < nit) {
          const int uw = min(it * 4 + ug, U - 1);
          const size_t o = ((size_t)n * U + (((need >> uw) & 1) ? uw : ufirst)) * kQ + 8 * ks;
          if constexpr (F32) {
            const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(P.emb) + o);
            const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(P.emb) + o + 4);
            e8[it][0] = a.x; e8[it][1] = a.y; e8[it][2] = a.z; e8[it][3] = a.w;
            e8[it][4] = b.x; e8[it][5] = b.y; e8[it][6] = b.z; e8[it][7] = b.w;
          } else {
            const dca::bf16x8 h = *reinterpret_cast<const dca::bf16x8*>(static_cast<const short*>(P.emb) + o);
#pragma unroll
            for (int j = 0; j < 8; ++j) e8[it][j] = dca::bf2f(h[j]);
          }
        }
    }
    if (lane < 32) s_zl[wv][lane] = zl;
    s_act[wv][lane] = a0; s_act[wv][lane + 64] = a1;
    s_msk[wv][lane] = m0; s_msk[wv][lane + 64] = m1;
    // ---- pointer logits q·emb_u, 4 units per wave-instruction (16 lanes × 8 features each)
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
      if (it < nit) {
        const int u = it * 4 + ug;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += q8[j] * e8[it][j];
        d = dca::group_sum<16>(d);
        if (ks == 0 && u < U) s_tl[wv][u] = d;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // ---- the four heads: (offset in flat action vector, width, source)
    const int hoff[4] = {0, 3, 12, 21};
    const int hw[4] = {3, 9, 9, U};
    float logp[4], pr[4], a[4];
    bool mk[4];
    float sel = 0.f;
    int nsel = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const bool in = lane < hw[h];
      float lg = 0.f;
      if (in) lg = (h == 3) ? s_tl[wv][lane] : s_zl[wv][hoff[h] + lane];
      mk[h] = in && s_msk[wv][hoff[h] + lane];
      a[h] = (in && s_act[wv][hoff[h] + lane]) ? 1.f : 0.f;
      head_lsm<PRECISE>(lg, mk[h], lane, hw[h], logp[h], pr[h]);
      if (!in) logp[h] = 0.f;
      const float sh = dca::wave_sum(a[h] * logp[h]);
      sel += sh;
      const int ns = __popcll(__ballot(a[h] > 0.f));
      nsel += ns;
      // entropy of this head over valid entries: -Σ m p logp
      acc[2 + h] += w_n * -dca::wave_sum(mk[h] ? pr[h] * logp[h] : 0.f);
    }
    const float valid = nsel > 0 ? 1.f : 0.f;
    const float V = s_zl[wv][21];
    const float R = R_n;
    float g_sel = 0.f, dV = 0.f;
    if (P.algo == 0) {   // PPO
      const float A = A_n;
      const float lr = sel - lpo_n;
      const float r = xexp<PRECISE>(lr);
      const float s1 = r * A;
      const float rc = fminf(fmaxf(r, 1.f - P.clip_eps), 1.f + P.clip_eps);
      const float s2 = rc * A;
      acc[0] += w_n * (valid * fminf(s1, s2));
      const bool clipped = (A > 0.f && r > 1.f + P.clip_eps) || (A < 0.f && r < 1.f - P.clip_eps);
      g_sel = clipped ? 0.f : w_n * (-valid * A * r * nm[0]);
      acc[1] += w_n * (valid * (V - R) * (V - R));
      dV = w_n * (P.vf_coef * 2.f * (V - R) * valid * nm[0]);
      acc[6] += valid * (-lr);
      acc[7] += valid * (fabsf(r - 1.f) > P.clip_eps ? 1.f : 0.f);
      acc[8] += valid * A;
    } else if (P.algo == 2) {   // off-policy PG with a truncated importance weight (replayed experience, V-trace style)
      // w = min(1, π/π_old) is a constant of the gradient: ∂/∂logπ of −w·A·logπ is −w·A (never zero, unlike the
      // clipped surrogate on experience many versions old); acc[7] counts the truncated rows
      const float A = A_n;
      const float lr = sel - lpo_n;
      const float r = xexp<PRECISE>(lr);
      const float w = fminf(r, 1.f);
      acc[0] += w_n * (valid * w * A);
      g_sel = w_n * (-valid * A * w * nm[0]);
      acc[1] += w_n * (valid * (V - R) * (V - R));
      dV = w_n * (P.vf_coef * 2.f * (V - R) * valid * nm[0]);
      acc[6] += valid * (-lr);
      acc[7] += valid * (r > 1.f ? 1.f : 0.f);
      acc[8] += valid * A;
    } else {             // VPG (reference objective)
      const float nr = nret_n;
      acc[0] += -sel * nr;
      g_sel = -nr * nm[1];
      acc[1] += (V - R) * (V - R);
      acc[9] += V;
      acc[10] += V * V;
      acc[8] += V - R;
      if (P.vf_coef > 0.f) {
        if (P.compat_value_bug) {
          const float S = (float)P.S_bug, Bq = (float)P.B_bug;
          dV = P.vf_coef * 2.f * (S * V - nm[6]) / (Bq * S * S);
        } else {
          dV = P.vf_coef * 2.f * (V - R) / ((float)P.S_bug * (float)P.B_bug);   // mean over ALL B·S rows (chunk-safe)
        }
      }
    }
    acc[11] += valid;
    if (P.logp_out) if (lane == 0) P.logp_out[n] = sel;
    // ---- gradients through the four log-softmaxes
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const bool in = lane < hw[h];
      float dlp = g_sel * a[h];
      // (w_n on the coefficient: the last product still contracts with the sum as it does without weights)
      if (P.ent_coef > 0.f) dlp += w_n * P.ent_coef * nm[2 + h] * (mk[h] ? pr[h] * (1.f + logp[h]) : 0.f);
      if (!in) dlp = 0.f;
      const float sd = dca::wave_sum(dlp);
      const float dl = dlp - (mk[h] ? pr[h] : 0.f) * sd;
      if (in) {
        if (h == 3) {
          s_dtl[wv][lane] = dl;
          P.dtl[(size_t)n * U + lane] = dl;
        } else {
          put_dz(P, (size_t)n * P.ldz + kQ + hoff[h] + lane, dl);
        }
      }
    }
    if (lane == 0) put_dz(P, (size_t)n * P.ldz + kQ + 21, dV);
    for (int c = kQ + 22 + lane; c < P.ldz; c += 64) put_dz(P, (size_t)n * P.ldz + c, 0.f);   // padding columns
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // ---- dq = Σ_u dtl[u] · emb[u]
    float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
      if (it < nit) {
        const int u = it * 4 + ug;
        const float g = (u < U) ? s_dtl[wv][u] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) dq[j] += g * e8[it][j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dq[j] += __shfl_xor(dq[j], 16, 64);
      dq[j] += __shfl_xor(dq[j], 32, 64);
    }
    if (ug == 0) {
      if (P.dz16) {
        dca::bf16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = dca::f2bf(dq[j]);
        *reinterpret_cast<dca::bf16x8*>(P.dz16 + (size_t)n * P.ldz + 8 * ks) = h;
      } else {
        float4* o = reinterpret_cast<float4*>(P.dz + (size_t)n * P.ldz + 8 * ks);
        o[0] = make_float4(dq[0], dq[1], dq[2], dq[3]);
        o[1] = make_float4(dq[4], dq[5], dq[6], dq[7]);
      }
    }
  }
  // ---- block partials
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kNPart; ++i) s_part[wv][i] = acc[i];
  }
  __syncthreads();
  if (tid < kNPart) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kRowsPerBlock; ++w) s += s_part[w][tid];
    P.part[(size_t)blockIdx.x * kNPart + tid] = s;
  }
}

}  // namespace

extern "C" int dca_heads_loss_nblocks(int N) { return (N + kRowsPerBlock - 1) / kRowsPerBlock; }

// emb_f32 = 1: emb is (N, U, 128) fp32, else bf16
extern "C" hipError_t dca_heads_loss(const float* z, int ldz, const void* emb, const unsigned char* act,
                                     const unsigned char* msk, int A, const float* adv, const float* ret,
                                     const float* logp_old, const float* nret, const float* norms, float* dz,
                                     float* dtl, float* part, float* logp_out, int N, int U, int algo,
                                     int compat_value_bug, int S_bug, int B_bug, float clip_eps, float ent_coef,
                                     float vf_coef, hipStream_t st, short* dz16, int emb_f32, int precise,
                                     const float* seqw, int B) {
  if (U > 64 || U < 1 || ldz < kQ + 22 || A != 21 + U) return hipErrorInvalidValue;
  // weights: PPO-family objectives only, and whole time steps of B sequences
  if (seqw && (algo == 1 || B < 1 || N % B != 0)) return hipErrorInvalidValue;
  Params P{z, ldz, emb, act, msk, A, adv, ret, logp_old, nret, norms, dz, dtl, part, logp_out, dz16, N, U, algo,
           compat_value_bug, S_bug, B_bug, clip_eps, ent_coef, vf_coef, seqw, B};
  if (emb_f32 && precise) heads_loss_kernel<true, true><<<dca_heads_loss_nblocks(N), 256, 0, st>>>(P);
  else if (emb_f32) heads_loss_kernel<true, false><<<dca_heads_loss_nblocks(N), 256, 0, st>>>(P);
  else heads_loss_kernel<false, false><<<dca_heads_loss_nblocks(N), 256, 0, st>>>(P);
  return hipGetLastError();
}
