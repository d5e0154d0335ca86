// XCD-team LSTM recurrence, backward. Team protocol, layouts, error codes (this kernel raises 2: a hand-off timed out)
// and the table of kernel forms: lstm_team.h.
//
// Every workgroup computes the recurrent gradient of its own units over the full K = 4H gate columns,
//   ∂h_t[b, J_m] = Σ_gc ∂G_{t+1}[b, gc] · W_hh[row(gc), J_m]      (gc = 4·j + q unit-major, row = q·H + j),
// its NWK waves each taking one K part (W_hhᵀ slice of the owned units in VGPRs), the partials summed through LDS
// (red[]). What a step hands to the other 31 workgroups is small: measured, an in-XCD hand-off is limited by the bytes
// WRITTEN per step (they also leave the XCD), not by the bytes read from L2 — a reduce-scatter of B×H partials per
// workgroup (512 KB per step per team at B=8, H=512) took 2.7 µs per hand-off.
//
// Exchange buffer xg, per team, [2 step parity][Bc rows][H units], tags t + 1 for step t:
//   Bf16Mfma              one 16-B chunk per (row, unit)  {bf16 d_i,d_f | tag | bf16 d_g,d_o | tag}
//   SplitMfma, VALU R > 1 two 16-B chunks                 {d_i, tag, d_f, tag} {d_g, tag, d_o, tag} (f32)
//   VALU R = 1 (HO)       one 8-B granule                 {f32 ∂h_t, tag}, in a prefix of the same buffer
//
// Iteration k (t = S - 1 - k), MFMA forms: prefetch the saved activations of the owned (row, unit) pairs → all
// threads poll ∂G_{t+1} into LDS (bf16; SplitMfma hi + lo) → barrier → each wave's MFMA product over its K quarter →
// red[] → barrier → owners sum the partials, add ∂L/∂h_t, compute the four gate gradients, publish them and store
// ∂gates.
// VALU forms of 2 / 4 / 8 rows (Valu4w; Valu8w at H = 512): the same, but wave wk polls only the chunks of its own K
// part into its private slice of the fp32 image dgf and goes straight to its pk_dot4 product: one barrier per step,
// red[] double-buffered by step parity (profiles/recurrence_wave_gather.md).
// One-row VALU forms — the ones that hand off ∂h (HO; profiles/recurrence_bwd_handoff.md): an owner publishes the
// {∂h_t, tag} granule right behind the reduction barrier; lane l of wave wk polls the granule of unit wk·UW + l,
// computes that unit's four gate gradients (gate_grads) from activations it prefetched, with the cell-gradient carry
// as per-lane state, and writes them into its wave's dgf slice; the lanes of the workgroup's own units store ∂gates
// and keep the bias sums. The forms of more rows stay on the ∂gates exchange (measured slower with the hand-off).
#include "lstm_team.h"

namespace {

// ∂h hand-off backward: the consumers' saved-activation loads are issued a step ahead, behind the gather (true), or at
// the top of the step that uses them, ahead of its poll (false)
constexpr bool kActsAhead = true;

// ∂L/∂pre-activations {d_i, d_f, d_g, d_o} of one (row, unit) at one step from ∂h_t (`dht`, recurrent part included),
// the saved activations gv = {i, f, g, o}, tc = tanh(c_t), cpv = c_{t-1}; advances the cell-gradient carry to step
// t - 1 and adds the four into `sum` (bias gradient). rcur: an episode starts at t (c_{t-1} is not read). The consumer
// side of the ∂h hand-off. These are the owner-side expressions below (dc = dcarry + dht·og·(1 − tc²), d_i = dc·gg·ig·
// (1 − ig), ...) in the same order, with the three places where the compiler fuses a multiply into an add there —
// 1 − tc², the add of dcarry, and the g and o bias sums; NOT 1 − gg², which it packs with 1 − og — written as fmaf
// and contraction switched off, so that what is computed here does not follow from how this context gets vectorised:
// bit for bit the owner-side results of every exact VALU form.
__device__ __forceinline__ dca::f32x4 gate_grads(const dca::f32x4 gv, float tc, float cpv, float dht, bool rcur,
                                                 float& dcarry, dca::f32x4& sum) {
#pragma clang fp contract(off)
  const float ig = gv[0], fg = gv[1], gg = gv[2], og = gv[3];
  const float dc = __builtin_fmaf(dht * og, __builtin_fmaf(-tc, tc, 1.f), dcarry);
  const float d_i = dc * gg * ig * (1.f - ig);
  const float d_f = rcur ? 0.f : dc * cpv * fg * (1.f - fg);
  const float qg = 1.f - gg * gg, qo = 1.f - og;
  const float pg = dc * ig, po = dht * tc * og;
  const float d_g = pg * qg;
  const float d_o = po * qo;
  dcarry = rcur ? 0.f : dc * fg;
  sum[0] += d_i;
  sum[1] += d_f;
  sum[2] = __builtin_fmaf(pg, qg, sum[2]);
  sum[3] = __builtin_fmaf(po, qo, sum[3]);
  return dca::f32x4{d_i, d_f, d_g, d_o};
}

// The form (P, ROWS, LIBM) and KS = H/128. In the body: V1 = an exact VALU form of R rows on NWK waves, MT = 16-row
// MFMA tiles per chain, F32 = fp32 W_hh and exchange, PREC = libm tanh, HO = the form hands off ∂h.
template <Prod P, int ROWS, int KS, bool LIBM>
__device__ __forceinline__ void lstm_team_bwd_body(
    const float* __restrict__ dhs, const float* __restrict__ gates4, const float* __restrict__ cs,
    const float* __restrict__ c0, const float* __restrict__ dhn, const float* __restrict__ dcn,
    const void* __restrict__ whh_, float* __restrict__ dgates4, float* __restrict__ dh0, float* __restrict__ dc0,
    i32x4* xg_all, TeamCtl* ctl, unsigned* err, int Btot, int Bc, int nch, int S, int sb, int st,
    unsigned long long* trace, short* __restrict__ dg16, float* __restrict__ dbpart, int knobs,
    const unsigned char* __restrict__ rst) {
  constexpr int H = 128 * KS;
  constexpr int U = H / kT;             // 4·KS units per workgroup (MFMA N, zero-padded to 16)
  constexpr bool F32 = P != Prod::Bf16Mfma;
  constexpr bool PREC = LIBM;
  constexpr bool V1 = is_valu(P);
  constexpr int VV = P == Prod::Valu4w ? 1 : (P == Prod::Valu8w ? 2 : 0);
  constexpr int MT = V1 ? 1 : ROWS / 16;
  constexpr int NT = form_threads(P);   // threads per workgroup
  constexpr int NWK = NT / 64;          // K parts = waves
  constexpr int KW = 4 * H / NWK;       // K (= 4H gate columns) per wave
  constexpr int KSTEP = KW / 32;
  constexpr int RB = MT * 16;
  constexpr int GP = 4 * H + 8;         // LDS pitch (bf16) of the gathered dG rows
  constexpr int KSL = KW / 16;          // V1: K slice per lane of a wave's K part
  constexpr int R = V1 ? ROWS : 1;      // V1: rows per chain (1, 2, 4, 8)
  constexpr int NPAIR = ((V1 ? R : RB) * U + NT - 1) / NT;
  // HO: the ∂h hand-off (see the file header). The one-row exact VALU forms whose wave covers at most 64 units of K —
  // one unit per lane. The two- and four-row forms exchange the gate gradients as before: every wave repeating the gate
  // math of 2 / 4 rows behind its poll measured slower in the learner rows that run them (learner_b16 8.535 → 8.580,
  // learner_b32 14.506 → 14.829, bptt350_learner 3.736 → 3.843 ms), and the four-row H = 128 form would also take 184
  // VGPRs against 153 (occupancy 3 → 2). So do the MFMA forms. The body below is written for R rows.
  constexpr int UW = KW / 4;            // units per wave's K part
  constexpr bool HO = V1 && UW <= 64 && R == 1;
  static_assert(V1 ? (R == 1 || R == 2 || R == 4 || R == 8) : (ROWS == 16 * MT && MT >= 1), "rows of the form");
  static_assert(!LIBM || (V1 && R == 1), "only the one-row VALU forms have libm activations");
  static_assert(VV != 2 || H == 512, "the eight-wave form is the H = 512 variant");
  static_assert(VV != 1 || H != 512, "at H = 512 the backward runs eight waves: Valu4w is not instantiated there");
  // (Measured and removed in round 5: ∂W_hh accumulated inside this recurrence — 128 accumulators per lane on every
  // step's critical path, 3755 vs 2091 µs for the backward, 7.03 vs 5.59 ms per learner step.)
  __shared__ short dgl[V1 ? 1 : RB][V1 ? 1 : GP];
  __shared__ short dglo[F32 && !V1 ? RB : 1][F32 && !V1 ? GP : 1];   // F32: lo bf16 half of the gathered dG
  // V1: dG_{t+1} of row 0, fp32, as 64 K slices each padded by 4 floats (bank spread, as forward)
  constexpr int SP = KSL + 4;
  constexpr int DROW = (4 * H / KSL) * SP;   // V1: floats per row image of dG_{t+1}
  __shared__ __attribute__((aligned(16))) float dgf[V1 ? R * DROW : 4];
  // partial products of the K parts. V1: R rows, two copies by step parity (see the hazard note in the step loop)
  constexpr int RR = V1 ? R : RB;
  __shared__ float red[V1 ? 2 : 1][NWK][RR][16 + 1];
  __shared__ float dbs[RB * U * 4];     // per-(row, unit, gate) bias-gradient sums of a chain
  __shared__ int sh_int;
  __shared__ unsigned sh_epoch;
  // packing: the chain's episode-start flags as a bit image (row b, step t → bit t of rbits[b·wpr + t/32]), built
  // once per chain. Byte loads of the flags at every step — two per owned pair, compared where they were issued —
  // measured +0.32 ms per B = 8, S = 1400 backward call on some boxes (1921 → 2244 µs, scripts/reset_probe.py);
  // chains with more than kRstWords·32 (row, step) flags read them from global memory as before.
  constexpr int kRstWords = 2048;
  __shared__ unsigned rbits[kRstWords];

  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int me = join_team(ctl, err, &sh_int, &sh_epoch);
  const unsigned epoch = sh_epoch;
  if (me < 0) return;
  const int team = me >> 6, m = me & 63;
  const int j0 = m * U;
  const int wpr = (S + 31) >> 5;        // flag words per row
  // 16-B chunks per (row, unit): bf16 {d_i,d_f | tag | d_g,d_o | tag}; F32 {d_i, tag, d_f, tag} {d_g, tag, d_o, tag}
  constexpr int CPU_ = F32 ? 2 : 1;
  i32x4* xg = xg_all + (size_t)team * 2 * Bc * H * CPU_;
#define TSTAMPB(ev)                                                                                       \
  if (trace && lane == 0 && wv < 4 && chain == 0 && k < 64)                                               \
    trace[(((size_t)m * 4 + wv) * 64 + k) * 8 + (ev)] = __builtin_amdgcn_s_memrealtime()

  if constexpr (!V1)
    for (int i = tid; i < RB * GP; i += NT) (&dgl[0][0])[i] = 0;
  if constexpr (F32 && !V1)
    for (int i = tid; i < RB * GP; i += NT) (&dglo[0][0])[i] = 0;

  // B operand: lane holds Wᵀ[gc][u] for gc = wv·H + ks·32 + 8·kg + j, u = lane & 15 (zero for u ≥ U)
  const int col = lane & 15, kg = lane >> 4;
  bf16x8 wf[V1 ? 1 : KSTEP];
  bf16x8 wfl[F32 && !V1 ? KSTEP : 1];
  float wq[V1 ? 4 * KSL : 1];
  if constexpr (V1) {
    // lane (ug = lane/16, slice = lane%16): W_hhᵀ of units j0 + 4·ug + uu (uu < 4) over the slice's gate columns
    // (wv < NWK, so wv / NWK = 0 and wv % NWK = wv here and below: written out because the compiler does not know the
    // bound, and folding it by hand changed the register allocation of all sixteen V1 backward kernels)
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int unit = 16 * (wv / NWK) + 4 * (lane >> 4) + uu;
#pragma unroll
      for (int j = 0; j < KSL; ++j) {
        const int gc = (wv % NWK) * KW + (lane & 15) * KSL + j;
        wq[uu * KSL + j] =
            (unit < U) ? static_cast<const float*>(whh_)[(size_t)((gc & 3) * H + (gc >> 2)) * H + j0 + unit] : 0.f;
      }
    }
  }
#pragma unroll
  for (int ks = 0; ks < (V1 ? 0 : KSTEP); ++ks) {
    bf16x8 v, vl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int gc = wv * KW + ks * 32 + 8 * kg + j;
      const size_t wi = (size_t)((gc & 3) * H + (gc >> 2)) * H + j0 + col;
      if constexpr (F32) {
        const float w = (col < U) ? static_cast<const float*>(whh_)[wi] : 0.f;
        v[j] = dca::f2bf(w);
        vl[j] = dca::f2bf(w - dca::bf2f(v[j]));
      } else {
        v[j] = (col < U) ? static_cast<const short*>(whh_)[wi] : (short)0;
      }
    }
    wf[ks] = v;
    if constexpr (F32 && !V1) wfl[ks] = vl;
  }

  // (Tried: one 16-B store instruction for the two hand-off chunks and the ∂gates record — lanes 16·r + u of wave 0
  // computing unit u redundantly, role r picking the record — the forward's merged-store idea applied here: 1.578 vs
  // 1.535 µs per step, slower; the three stores of the 16 unit lanes stay.)
  unsigned spins = 0;
  unsigned long long since = 0;
  for (unsigned iter = 0;; ++iter) {
    const int chain = next_chain(ctl, team, m, iter, nch, &sh_int);
    if (chain < 0) break;
    const int b0 = chain * Bc;
    const int B = min(Bc, Btot - b0);
    const unsigned tagbase = make_tagbase(epoch, iter);
    const bool rl = rst != nullptr && B * wpr <= kRstWords;    // flags from the LDS bit image
    if (rl) {
      for (int w = tid; w < B * wpr; w += NT) {
        const int b = w / wpr, tb = (w - b * wpr) * 32;
        const unsigned char* fr = rst + (size_t)(b0 + b) * sb;
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j)
          if (tb + j < S) v |= (fr[(size_t)(tb + j) * st] != 0 ? 1u : 0u) << j;
        rbits[w] = v;
      }
      lds_barrier();
    }
    float dcarry[NPAIR];
    dca::f32x4 dsum[NPAIR];               // Σ_t ∂gates of the owned pairs (bias gradient)
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) dsum[i] = dca::f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      const int pi = tid + NT * i;
      dcarry[i] = (pi < B * U && dcn) ? dcn[(size_t)(b0 + pi / U) * H + j0 + pi % U] : 0.f;
    }
    // HO: lane `lane` of wave wk handles unit cu = wk·UW + lane of every row — it polls that unit's ∂h granule, turns
    // it into the unit's four gate gradients and writes them into the wave's slice of dgf. Per handled (row, unit):
    // the saved activations of the step gathered next (cg = gates4, ccv = c, ccp = c of the step before it, ctc =
    // tanh(ccv)), the cell-gradient carry, and — used by the lanes of this workgroup's own units only — Σ_t ∂gates.
    constexpr int RH = HO ? R : 1;
    const int cu = (wv % NWK) * UW + lane;
    const bool hasu = HO && lane < UW;
    const bool mine = hasu && cu >= j0 && cu < j0 + U;
    dca::f32x4 cg[RH], csum[RH];
    float ccv[RH], ccp[RH], ctc[RH], cdc[RH];
    bool crc[RH];
    // saved activations of step s for the handled pairs (ccv is carried over: c of step s was ccp of step s + 1)
    auto load_acts = [&](int s) {
#pragma unroll
      for (int r = 0; r < RH; ++r) {
        if (r < B && hasu) {
          const size_t bt = (size_t)(b0 + r) * sb + (size_t)s * st;
          cg[r] = *reinterpret_cast<const dca::f32x4*>(gates4 + (bt * H + cu) * 4);
          ccp[r] = s > 0 ? cs[(bt - st) * H + cu] : c0[(size_t)(b0 + r) * H + cu];
        }
      }
    };
    if constexpr (HO) {
#pragma unroll
      for (int r = 0; r < RH; ++r) {
        const bool on = r < B && hasu;
        csum[r] = dca::f32x4{0.f, 0.f, 0.f, 0.f};
        cg[r] = dca::f32x4{0.f, 0.f, 0.f, 0.f};
        ccp[r] = ctc[r] = 0.f;
        crc[r] = false;
        cdc[r] = (on && dcn) ? dcn[(size_t)(b0 + r) * H + cu] : 0.f;
        ccv[r] = on ? cs[((size_t)(b0 + r) * sb + (size_t)(S - 1) * st) * H + cu] : 0.f;
        // land this load here: left pending into the step loop, the compiler's wait-count merge at the loop header
        // takes ccv for a load in flight in EVERY iteration and drains vmcnt — the publish, the ∂L/∂h load and the
        // activation loads issued a step ahead — in front of each step's tanh and first poll
        asm volatile("" ::"v"(ccv[r]));
      }
    }
    bool dead = false;
    for (int k = 0; k <= S; ++k) {
      const int t = S - 1 - k;          // step whose ∂h (HO) / gate gradients are published this iteration (-1: final)
      spins = 0;
      since = 0;
      TSTAMPB(0);
      // ---- prefetch the saved activations of step t for the owned pairs
      dca::f32x4 gv[NPAIR];
      float cv[NPAIR], cpv[NPAIR], dv[NPAIR], dvl[NPAIR];
      bool rcur[NPAIR], rnext[NPAIR];     // packing: episode starts at t (c_{t-1} unused) / at t+1 (h_t unused by t+1)
      if constexpr (HO) {
        // owners: ∂L/∂h_t from above and the start flag of t + 1. Consumers: tanh(c) and the start flag of the step
        // gathered below (t + 1), and its activations unless they were issued a step ahead.
        if (t >= 0) {
#pragma unroll
          for (int i = 0; i < NPAIR; ++i) {
            const int pi = tid + NT * i;
            rnext[i] = false;
            if (pi < B * U) {
              const int b = pi / U, u = pi % U;
              const size_t bt = (size_t)(b0 + b) * sb + (size_t)t * st;
              dv[i] = dhs[bt * H + j0 + u];
              if (rl) rnext[i] = t + 1 < S && ((rbits[b * wpr + ((t + 1) >> 5)] >> ((t + 1) & 31)) & 1u);
              else if (rst != nullptr) rnext[i] = t + 1 < S && rst[bt + st] != 0;
            }
          }
        }
        if (k > 0) {
          if constexpr (!kActsAhead) load_acts(t + 1);
#pragma unroll
          for (int r = 0; r < RH; ++r) {
            if (r < B && hasu) {
              ctc[r] = tanh_<PREC>(ccv[r]);
              if (rl) crc[r] = (rbits[r * wpr + ((t + 1) >> 5)] >> ((t + 1) & 31)) & 1u;
              else if (rst != nullptr) crc[r] = rst[(size_t)(b0 + r) * sb + (size_t)(t + 1) * st] != 0;
            }
          }
        } else if constexpr (kActsAhead) {
          load_acts(t);
        }
      } else {
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
          const int pi = tid + NT * i;
          rcur[i] = rnext[i] = false;
          gv[i] = dca::f32x4{0.f, 0.f, 0.f, 0.f};       // (defined on every path: every thread lands them below)
          cv[i] = cpv[i] = dv[i] = 0.f;
          if (t >= 0 && pi < B * U) {
            const int b = pi / U, u = pi % U;
            const size_t bt = (size_t)(b0 + b) * sb + (size_t)t * st;
            gv[i] = *reinterpret_cast<const dca::f32x4*>(gates4 + (bt * H + j0 + u) * 4);
            cv[i] = cs[bt * H + j0 + u];
            cpv[i] = t > 0 ? cs[(bt - st) * H + j0 + u] : c0[(size_t)(b0 + b) * H + j0 + u];
            dv[i] = dhs[bt * H + j0 + u];
            if (rl) {
              const unsigned* rw = rbits + b * wpr;
              rcur[i] = (rw[t >> 5] >> (t & 31)) & 1u;
              rnext[i] = t + 1 < S && ((rw[(t + 1) >> 5] >> ((t + 1) & 31)) & 1u);
            } else if (rst != nullptr) {
              rcur[i] = rst[bt] != 0;
              rnext[i] = t + 1 < S && rst[bt + st] != 0;
            }
          }
        }
      }
      // ---- gather dG_{t+1} (B × 4H bf16) into LDS, all loads of a group of 8 rows in flight
      if (k > 0) {
        const unsigned tag = tagbase | (unsigned)(t + 2);
        const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(xg + (size_t)((t + 1) & 1) * Bc * H * CPU_, Bc * H * CPU_ * 16);
        constexpr int RG = F32 ? 4 : 8;                    // rows per gather group
        constexpr int NL = RG * H * CPU_ / NT;             // chunks per thread per group
        if constexpr (HO) {
          // ∂h hand-off: one 8-byte {∂h_{t+1}, tag} granule per (row, unit), a quarter of the bytes of the gate-gradient
          // chunks, written and polled. The lane polls the granule of its unit, computes the unit's four gate
          // gradients (the owner used to, ahead of its publish) and writes them as one 16-byte ds_write into its
          // wave's slice of dgf — still exactly the columns the wave's product reads and nothing else reads.
          const __amdgpu_buffer_rsrc_t rh =
              uniform_rsrc(reinterpret_cast<const char*>(xg) + (size_t)((t + 1) & 1) * Bc * H * 8, Bc * H * 8);
          u32x2 g[RH];
          bool okc[RH];
#pragma unroll
          for (int r = 0; r < RH; ++r) {
            okc[r] = r >= B || !hasu;
            g[r] = u32x2{0u, 0u};
          }
          while (true) {
#pragma unroll
            for (int r = 0; r < RH; ++r)
              if (!okc[r]) g[r] = __builtin_amdgcn_raw_buffer_load_b64(rh, (r * H + cu) * 8, 0, kSc1);
            bool ok = true;
#pragma unroll
            for (int r = 0; r < RH; ++r) {
              okc[r] = okc[r] || g[r].y == tag;
              ok &= okc[r];
            }
            if (__all(ok)) break;
            if (spin_fail(spins, since, ctl, err, 2u, knobs)) { dead = true; break; }
          }
          // The owners' ∂L/∂h_t landed with the poll (returns are in order). Moved to a register the compiler has
          // seen no load into: the wait it otherwise emits ahead of the publish, at the join with the k = 0 path, is
          // vmcnt(0) and covers the activation loads issued below.
#pragma unroll
          for (int i = 0; i < NPAIR; ++i) asm volatile("v_mov_b32 %0, %1" : "=v"(dvl[i]) : "v"(dv[i]));
          if (!dead) {
#pragma unroll
            for (int r = 0; r < RH; ++r) {
              if (r < B && hasu) {
                const dca::f32x4 d =
                    gate_grads(cg[r], ctc[r], ccp[r], __uint_as_float(g[r].x), crc[r], cdc[r], csum[r]);
                constexpr int gpl = KSL / 4;                 // units per K slice
                *reinterpret_cast<dca::f32x4*>(&dgf[r * DROW + (cu / gpl) * SP + (cu % gpl) * 4]) = d;
                if (mine) {
                  const size_t bt = (size_t)(b0 + r) * sb + (size_t)(t + 1) * st;
                  *reinterpret_cast<dca::f32x4*>(dgates4 + (bt * H + cu) * 4) = d;
                  if (t + 1 == 0) dc0[(size_t)(b0 + r) * H + cu] = cdc[r];
                }
                ccv[r] = ccp[r];
              }
            }
            if constexpr (kActsAhead)
              if (t >= 0) load_acts(t);
          }
          TSTAMPB(5);
        } else if constexpr (V1) {
          // Wave-private gather: wave wk polls, tag-checks and writes to LDS exactly the chunks of ITS K part — for
          // every row the chunks r ∈ [wk·KW/2, (wk+1)·KW/2), gate columns gc = 2r ∈ [wk·KW, (wk+1)·KW) — which are
          // the 16 slices (wk·16 + slice)·SP its product reads and nothing else reads. CW chunks per lane per row,
          // the same count per lane as a tid + NT·i split of the row.
          constexpr int CW = KW / 128;                     // chunks per lane per row
          constexpr int NLW = R * CW;
          static_assert(KW % 128 == 0, "a wave's K part is whole rounds of 64 chunks");
          const int cw0 = (wv % NWK) * (KW / 2) + lane;    // this lane's first chunk of a row
          i32x4 g[NLW];
          bool okc[NLW];
#pragma unroll
          for (int i = 0; i < NLW; ++i) okc[i] = i / CW >= B;
          while (true) {
#pragma unroll
            for (int i = 0; i < NLW; ++i)
              if (!okc[i])
                g[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((i / CW) * H * CPU_ + cw0 + 64 * (i % CW)) * 16, 0, kSc1);
            bool ok = true;
#pragma unroll
            for (int i = 0; i < NLW; ++i) {
              okc[i] = okc[i] || (((unsigned)g[i].y == tag) & ((unsigned)g[i].w == tag));
              ok &= okc[i];
            }
            if (__all(ok)) break;
            if (spin_fail(spins, since, ctl, err, 2u, knobs)) { dead = true; break; }
          }
#pragma unroll
          for (int i = 0; i < NLW; ++i) {
            if (i / CW < B) {
              const int r = cw0 + 64 * (i % CW), gc = 4 * (r >> 1) + 2 * (r & 1);
              *reinterpret_cast<float2*>(&dgf[(i / CW) * DROW + (gc / KSL) * SP + gc % KSL]) =
                  make_float2(__int_as_float(g[i].x), __int_as_float(g[i].z));
            }
          }
        } else {
          for (int g0 = 0; g0 < B && !dead; g0 += RG) {
            const int nck = min(RG, B - g0) * H * CPU_;
            i32x4 g[NL];
            bool okc[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i) okc[i] = tid + NT * i >= nck;
            while (true) {
#pragma unroll
              for (int i = 0; i < NL; ++i)
                if (!okc[i]) g[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (g0 * H * CPU_ + tid + NT * i) * 16, 0, kSc1);
              bool ok = true;
#pragma unroll
              for (int i = 0; i < NL; ++i) {
                okc[i] = okc[i] || (((unsigned)g[i].y == tag) & ((unsigned)g[i].w == tag));
                ok &= okc[i];
              }
              if (__all(ok)) break;
              if (spin_fail(spins, since, ctl, err, 2u, knobs)) { dead = true; break; }
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
              const int ci = tid + NT * i;
              if (ci < nck) {
                if constexpr (F32) {
                  const int b = g0 + ci / (2 * H), r = ci % (2 * H), gc = 4 * (r >> 1) + 2 * (r & 1);
                  const float x = __int_as_float(g[i].x), z = __int_as_float(g[i].z);
                  const short xh = dca::f2bf(x), zh = dca::f2bf(z);
                  *reinterpret_cast<unsigned*>(&dgl[b][gc]) = (unsigned)(unsigned short)xh | ((unsigned)(unsigned short)zh << 16);
                  *reinterpret_cast<unsigned*>(&dglo[b][gc]) =
                      (unsigned)(unsigned short)dca::f2bf(x - dca::bf2f(xh)) |
                      ((unsigned)(unsigned short)dca::f2bf(z - dca::bf2f(zh)) << 16);
                } else {
                  const int b = g0 + ci / H, j = ci % H;
                  *reinterpret_cast<u32x2*>(&dgl[b][4 * j]) = u32x2{(unsigned)g[i].x, (unsigned)g[i].z};
                }
              }
            }
          }
        }
      }
      // The forms on the ∂gates exchange: land the step's activation prefetch here, behind the gather, as the forward
      // lands its own (lstm_team_fwd.hip). A polling thread has just waited vmcnt(0), so nothing is outstanding; left
      // to the compiler, "may be in flight" goes round the back edge and the next step's loads into these registers
      // wait out all but the last three of this step's stores at the top of the step. Outside any branch.
      if constexpr (!HO) {
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) asm volatile("" ::"v"(gv[i]), "v"(cv[i]), "v"(cpv[i]), "v"(dv[i]));
      }
      TSTAMPB(1);
      if constexpr (V1) {
        // No workgroup barrier here (the MFMA forms below keep theirs). Hazards:
        // * dgf: wave wk wrote the slices [wk·16, wk·16 + 16) of every row image from chunks it polled itself, and its
        //   product below reads exactly those slices — no wave reads another wave's region, so the image is
        //   wave-private and only the wave's own ds_writes have to land before its ds_reads: lgkmcnt(0). The next
        //   step's writes follow this step's reads in the same wave's program order.
        // * red[]: double-buffered by step parity. Without this barrier nothing orders a wave's product of step k + 1
        //   behind the pair-owning threads' reads of step k: those threads' publish depends on `rec`, but a wave whose
        //   K part holds none of this workgroup's units completes its next gather on OTHER workgroups' publishes
        //   alone. So step k + 1 writes red[(k + 1) & 1] while step k's sums may still be read from red[k & 1]; a write
        //   to red[k & 1] again (step k + 2) lies behind barrier 2 of step k + 1, which every pair-owning thread
        //   reaches only after its reads of step k returned (lds_barrier waits lgkmcnt(0) first).
        // * barriers per step: exactly one (barrier 2) for every wave in every iteration — k = 0 (no gather, no
        //   product), the clean path, a wave whose gather gave up (it skips the product, raises sh_int and still
        //   arrives), and k = S (dh0). Everybody leaves the loop behind barrier 2 of the same iteration. (sh_int is
        //   only ever raised, and the launch ends behind it: a wave that read it late — after a dead wave of the NEXT
        //   iteration raised it — leaves one iteration early, and its team_exit barrier pairs with the others'
        //   barrier 2.)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      } else {
        if (dead) sh_int = -2;
        lds_barrier();
        if (sh_int == -2) break;
        TSTAMPB(2);
      }
      // ---- partial recurrent gradient over this wave's K quarter → red[wv]
      const int rp = V1 ? (k & 1) : 0;
      if (V1 && k > 0) {
       if (!dead) {
        const int wk = wv % NWK;
        const int u0 = 16 * (wv / NWK) + 4 * (lane >> 4);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r >= B) break;                                  // (B is uniform)
          float o0, o1, o2, o3;
          const float* x = &dgf[r * DROW + (wk * 16 + (lane & 15)) * SP];
          pk_dot4<KSL>(wq, x, o0, o1, o2, o3);
          o0 = row_sum16(o0);
          o1 = row_sum16(o1);
          o2 = row_sum16(o2);
          o3 = row_sum16(o3);
          if ((lane & 15) == 0 && u0 < U) {
            red[rp][wk][r][u0] = o0;
            red[rp][wk][r][u0 + 1] = o1;
            red[rp][wk][r][u0 + 2] = o2;
            red[rp][wk][r][u0 + 3] = o3;
          }
        }
       }
      } else if (k > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (mt * 16 >= B) break;
          dca::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if constexpr (F32) {
            dca::f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEP; ++ks) {
              const bf16x8 a = *reinterpret_cast<const bf16x8*>(&dgl[mt * 16 + col][wv * KW + ks * 32 + 8 * kg]);
              const bf16x8 al = *reinterpret_cast<const bf16x8*>(&dglo[mt * 16 + col][wv * KW + ks * 32 + 8 * kg]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ks], acc, 0, 0, 0);
              a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[ks], a1, 0, 0, 0);
              a2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wfl[ks], a2, 0, 0, 0);
            }
            acc += a1 + a2;
          } else {
#pragma unroll
            for (int ks = 0; ks < KSTEP; ++ks) {
              const bf16x8 a = *reinterpret_cast<const bf16x8*>(&dgl[mt * 16 + col][wv * KW + ks * 32 + 8 * kg]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ks], acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) red[0][wv][mt * 16 + kg * 4 + r][col] = acc[r];
        }
      }
      TSTAMPB(3);
      if (V1 && dead) sh_int = -2;
      lds_barrier();
      if (V1 && sh_int == -2) break;
      TSTAMPB(4);
      if (t < 0) {
        for (int i = tid; i < B * U; i += NT) {
          const int b = i / U, u = i % U;
          float acc = 0.f;
#pragma unroll
          for (int w = 0; w < NWK; ++w) acc += red[rp][w][b][u];
          // an episode starting at step 0 never read h0
          dh0[(size_t)(b0 + b) * H + j0 + u] = (rst != nullptr && rst[(size_t)(b0 + b) * sb] != 0) ? 0.f : acc;
        }
        break;
      }
      // ---- gate gradients for the owned (row, unit) pairs; publish dG_t, write ∂gates
      const __amdgpu_buffer_rsrc_t ws = uniform_rsrc(xg + (size_t)(t & 1) * Bc * H * CPU_, Bc * H * CPU_ * 16);
      const int tg = (int)(tagbase | (unsigned)(t + 1));
      if constexpr (HO) {
        // ---- owners: ∂h_t = ∂L/∂h_t + recurrent part, published at once; the gate gradients are the consumers' work
        const __amdgpu_buffer_rsrc_t wh =
            uniform_rsrc(reinterpret_cast<const char*>(xg) + (size_t)(t & 1) * Bc * H * 8, Bc * H * 8);
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
          const int pi = tid + NT * i;
          if (pi < B * U) {
            const int b = pi / U, u = pi % U;
            float rec = 0.f;
            if (k == 0) {
              rec = dhn ? dhn[(size_t)(b0 + b) * H + j0 + u] : 0.f;
              // no gather in this iteration: the one publish that waits for memory waits in this branch (see dvl)
              asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(dvl[i]), "=v"(rec) : "v"(dv[i]), "v"(rec));
            } else if (!rnext[i]) {
#pragma unroll
              for (int w = 0; w < NWK; ++w) rec += red[rp][w][b][u];
            }
            const float dht = dvl[i] + rec;
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(dht), (unsigned)tg}, wh, (b * H + j0 + u) * 8, 0,
                                                  kPlain);
          }
        }
      } else {
#pragma unroll
      for (int i = 0; i < NPAIR; ++i) {
        const int pi = tid + NT * i;
        if (pi < B * U) {
          const int b = pi / U, u = pi % U;
          float rec = 0.f;
          if (k == 0) {
            rec = dhn ? dhn[(size_t)(b0 + b) * H + j0 + u] : 0.f;
          } else if (!rnext[i]) {
#pragma unroll
            for (int w = 0; w < NWK; ++w) rec += red[rp][w][b][u];
          }
          const float ig = gv[i][0], fg = gv[i][1], gg = gv[i][2], og = gv[i][3];
          const float dht = dv[i] + rec;
          const float tc = tanh_<PREC>(cv[i]);
          const float dc = dcarry[i] + dht * og * (1.f - tc * tc);
          const float d_i = dc * gg * ig * (1.f - ig);
          const float d_f = rcur[i] ? 0.f : dc * cpv[i] * fg * (1.f - fg);
          const float d_g = dc * ig * (1.f - gg * gg);
          const float d_o = dht * tc * og * (1.f - og);
          dcarry[i] = rcur[i] ? 0.f : dc * fg;
          const size_t bt = (size_t)(b0 + b) * sb + (size_t)t * st;
          if constexpr (F32) {
            const int o = (b * H + j0 + u) * 2 * 16;
            __builtin_amdgcn_raw_buffer_store_b128(i32x4{__float_as_int(d_i), tg, __float_as_int(d_f), tg}, ws, o, 0,
                                                   kPlain);
            __builtin_amdgcn_raw_buffer_store_b128(i32x4{__float_as_int(d_g), tg, __float_as_int(d_o), tg}, ws, o + 16,
                                                   0, kPlain);
            *reinterpret_cast<dca::f32x4*>(dgates4 + (bt * H + j0 + u) * 4) = dca::f32x4{d_i, d_f, d_g, d_o};
          } else {
            const unsigned p01 = (unsigned)(unsigned short)dca::f2bf(d_i) | ((unsigned)(unsigned short)dca::f2bf(d_f) << 16);
            const unsigned p23 = (unsigned)(unsigned short)dca::f2bf(d_g) | ((unsigned)(unsigned short)dca::f2bf(d_o) << 16);
            __builtin_amdgcn_raw_buffer_store_b128(i32x4{(int)p01, tg, (int)p23, tg}, ws, (b * H + j0 + u) * 16, 0, kPlain);
            if (dg16) *reinterpret_cast<u32x2*>(dg16 + (bt * H + j0 + u) * 4) = u32x2{p01, p23};
            else *reinterpret_cast<dca::f32x4*>(dgates4 + (bt * H + j0 + u) * 4) = dca::f32x4{d_i, d_f, d_g, d_o};
          }
          dsum[i] += dca::f32x4{d_i, d_f, d_g, d_o};
          if (t == 0) dc0[(size_t)(b0 + b) * H + j0 + u] = dcarry[i];
        }
      }
      }
      TSTAMPB(6);
    }
    if (sh_int == -2) return;
    if (dbpart) {
      // bias gradient of this chain for the owned units: Σ over rows (fixed order) of the per-pair sums
      if constexpr (HO) {
#pragma unroll
        for (int r = 0; r < RH; ++r)
          if (r < B && mine) *reinterpret_cast<dca::f32x4*>(&dbs[(r * U + cu - j0) * 4]) = csum[r];
      } else {
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
          const int pi = tid + NT * i;
          if (pi < B * U) *reinterpret_cast<dca::f32x4*>(&dbs[pi * 4]) = dsum[i];
        }
      }
      __syncthreads();
      for (int o = tid; o < U * 4; o += NT) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dbs[b * U * 4 + o];
        // PyTorch's gate-major order (gate q of unit j at q·H + j): the partials' chain sum IS ∂b_ih = ∂b_hh
        dbpart[(size_t)chain * 4 * H + (o & 3) * H + j0 + (o >> 2)] = acc;
      }
    }
    __syncthreads();
    if (tid == 0) add_agent(&ctl->done[team], 1u);
  }
#undef TSTAMPB
}

template <Prod P, int ROWS, int KS, bool LIBM>
__global__ __launch_bounds__(form_threads(P), 1) void lstm_team_bwd_kernel(
    const float* __restrict__ dhs, const float* __restrict__ gates4, const float* __restrict__ cs,
    const float* __restrict__ c0, const float* __restrict__ dhn, const float* __restrict__ dcn,
    const void* __restrict__ whh, float* __restrict__ dgates4, float* __restrict__ dh0, float* __restrict__ dc0,
    i32x4* xg_all, TeamCtl* ctl, unsigned* err, int Btot, int Bc, int nch, int S, int sb, int st,
    unsigned long long* trace, short* __restrict__ dg16, float* __restrict__ dbpart, int knobs,
    const unsigned char* __restrict__ rst) {
  __builtin_amdgcn_s_setprio(3);
  lstm_team_bwd_body<P, ROWS, KS, LIBM>(dhs, gates4, cs, c0, dhn, dcn, whh, dgates4, dh0, dc0, xg_all, ctl, err, Btot, Bc, nch,
                             S, sb, st, trace, dg16, dbpart, knobs, rst);
  team_exit(ctl, err, nch);
}

}  // namespace

extern "C" hipError_t dca_lstm_team_bwd(const float* dhs, const float* gates4, const float* cs, const float* c0,
                                        const float* dhn, const float* dcn, const void* whh, float* dgates4,
                                        float* dh0, float* dc0, void* ctl_mem, void* ws, size_t ws_bytes,
                                        unsigned* err, int B, int S, int H, int time_major, hipStream_t stream,
                                        unsigned long long* trace, short* dg16, float* dbpart, int f32, int precise,
                                        const unsigned char* rst, int exact, int rows) {
  if (B < 1 || S < 1 || S >= 65534 || (H != 128 && H != 256 && H != 512)) return hipErrorInvalidValue;
  if (dgates4 == nullptr && dg16 == nullptr) return hipErrorInvalidValue;
  if (f32 && dgates4 == nullptr) return hipErrorInvalidValue;
  int nch, Bc, MT;
  if (!plan_any(B, f32, exact, rows, nch, Bc, MT)) return hipErrorInvalidValue;
  if (ws_bytes < dca_lstm_team_workspace(B, H, 1, f32, exact, rows) || ctl_mem == nullptr) return hipErrorInvalidValue;
  const int sb = time_major ? 1 : S, st = time_major ? B : 1;
  TeamCtl* ctl = reinterpret_cast<TeamCtl*>(ctl_mem);
  i32x4* xb = reinterpret_cast<i32x4*>(ws);
  const Form form = select_form(f32 != 0, Bc, H, true, precise != 0, exact != 0);
#define DCA_B(P, ROWS, H_, LIBM)                                                                                \
  if (form == Form{Prod::P, ROWS, H_, LIBM}) {                                                                  \
    lstm_team_bwd_kernel<Prod::P, ROWS, H_ / 128, LIBM><<<kMaxTeams * kT, form_threads(Prod::P), 0, stream>>>(  \
        dhs, gates4, cs, c0, dhn, dcn, whh, dgates4, dh0, dc0, xb, ctl, err, B, Bc, nch, S, sb, st, trace, dg16, \
        dbpart, team_knobs(), rst);                                                                             \
    return hipGetLastError();                                                                                   \
  }
  DCA_TEAM_BWD_FORMS(DCA_B)
#undef DCA_B
  return hipErrorInvalidValue;           // kNoForm
}
