// XCD-team LSTM recurrence, forward. Team protocol, layouts, error codes (this kernel raises 1: a hand-off timed out)
// and the table of kernel forms: lstm_team.h.
//
// Exchange buffer xg, per team: [2 step parity][Bc rows] granules of 8 bytes {payload, tag} — bf16 weights: H/2 per
// row, {2 × bf16 h, tag}; fp32 weights: H per row, {f32 h, tag}. h_t is written to parity t & 1 with tag t + 1.
//
// A step t, MFMA forms (Bf16Mfma, SplitMfma): all 256 threads poll h_{t-1} (16-byte chunks, each re-polled only until
// its tags match) into LDS as bf16 (SplitMfma: a hi and a lo image) → barrier → waves w < U/4 each own one 16-column
// tile = 4 units × 4 gates over the full K = H, their W_hh slice in VGPRs (SplitMfma: hi·hi + lo·hi + hi·lo) → a 4×4
// quad transpose puts (i, f, g, o) of one (row, unit) in one lane → cell update, c in registers → publish the h_t
// granule → store h, c and the activated gates.
// A step t, VALU forms (Valu4w, 1 / 2 / 4 / 8 rows): the same poll, into fp32 row images of 16 padded K slices →
// barrier → lane (unit, slice) of a unit-owning wave holds the 4 gate rows of its unit over its slice (4·H/16 fp32
// VGPRs) and runs pk_dot4 per row, row_sum16 sums the 16 slices into every lane of the unit's group → activations and
// cell update for every row in every lane of the group (8 rows: one row at a time) → the slice-r lane publishes row
// r's granule → c and h leave in one store instruction (slice 2r: row r's c and gates, slice 2r + 1: its h).
// Waits on vector memory in a step, every form: the poll's, those of the t = 0 copy and the time-out path, and one
// landing of the step's prefetch behind the gather (free behind a poll). None between a step's stores and the next
// step's first poll: until profiles/recurrence_fwd_waits.md the compiler placed two vmcnt(0) per step for a chain-start
// load left pending (scripts/asm_step_waits.py lists them), and every forward measurement older than that carried them.
#include "lstm_team.h"

namespace {

// 8 consecutive fp32 values → hi / lo bf16 fragments (x = hi + lo up to ≈2⁻¹⁷ relative)
__device__ __forceinline__ void split_frag(const float* __restrict__ p, bf16x8& hi, bf16x8& lo) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hi[j] = dca::f2bf(v[j]);
    lo[j] = dca::f2bf(v[j] - dca::bf2f(hi[j]));
  }
}

// The form (P, ROWS, LIBM) and KS = H/128. In the body: V1 = an exact VALU form of R rows, MT = 16-row MFMA tiles per
// chain (Bc ≤ 16·MT), F32 = fp32 W_hh and h exchange, PREC = libm activations.
template <Prod P, int ROWS, int KS, bool LIBM>
__device__ __forceinline__ void lstm_team_fwd_body(
    const float* __restrict__ xp4, const void* __restrict__ whh_, const float* __restrict__ h0,
    const float* __restrict__ c0, short* __restrict__ hs, float* __restrict__ hsf, float* __restrict__ cs,
    float* __restrict__ gates4, float* __restrict__ hn, float* __restrict__ cn, unsigned long long* xg_all,
    TeamCtl* ctl, unsigned* err, int Btot, int Bc, int nch, int S, int sb, int st, unsigned long long* trace,
    int knobs, const float* __restrict__ bias4, const unsigned char* __restrict__ rst) {
  constexpr int H = 128 * KS;
  constexpr int U = H / kT;             // units per workgroup (4·KS)
  constexpr int NTILE = U / 4;          // 16-column MFMA tiles per workgroup (= KS)
  constexpr int KSTEP = H / 32;         // k-steps of the full K
  constexpr int HP = H + 8;             // LDS row pitch (bf16)
  static_assert(P != Prod::Valu8w, "the forward has no eight-wave form (slower at every measurement, see lstm_team.h)");
  constexpr bool F32 = P != Prod::Bf16Mfma;
  constexpr bool PREC = LIBM;
  constexpr bool V1 = is_valu(P);
  constexpr int MT = V1 ? 1 : ROWS / 16;
  constexpr int RB = MT * 16;
  constexpr int NT = form_threads(P);             // threads per workgroup
  constexpr int LPU = 16;                         // V1: lanes (K slices) per unit
  constexpr int UPW = 64 / LPU;                   // V1: units per wave
  constexpr int KSL = H / LPU;                    // V1: K slice per lane
  constexpr int R = V1 ? ROWS : 1;                // V1: rows per chain (1, 2, 4, 8)
  constexpr int NR = V1 ? R : MT;                 // per-lane row registers (V1: every row; MFMA: one per tile)
  static_assert(V1 ? (R == 1 || R == 2 || R == 4 || R == 8) : (ROWS == 16 * MT && MT >= 1), "rows of the form");
  static_assert(!LIBM || (V1 && R == 1), "only the one-row VALU forms have libm activations");
  __shared__ short hl[V1 ? 1 : 2][V1 ? 1 : RB][V1 ? 1 : HP];
  __shared__ short hlo[F32 && !V1 ? 2 : 1][F32 && !V1 ? RB : 1][F32 && !V1 ? HP : 1];   // F32: lo bf16 half of h
  // V1: h_{t-1} of each row as 16 K slices, each padded by 4 floats (the 16 lanes of a row read 16 different slices
  // with one ds_read_b128: unpadded 128-B strides would put pairs of lanes on the same banks)
  constexpr int SP = KSL + 4;
  constexpr int ROWF = LPU * SP;                  // V1: floats per row image
  __shared__ __attribute__((aligned(16))) float hf[V1 ? 2 : 1][V1 ? R * ROWF : 4];
  __shared__ int sh_int;
  __shared__ unsigned sh_epoch;

  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int me = join_team(ctl, err, &sh_int, &sh_epoch, (knobs >> 11) & 1);
  const unsigned epoch = sh_epoch;
  if (me < 0) return;
  const int team = me >> 6, m = me & 63;
  const int j0 = m * U;
#define TSTAMP(ev)                                                                                        \
  if (trace && lane == 0 && wv < 4 && chain == 0 && t < 64)                                                \
    trace[(((size_t)m * 4 + wv) * 64 + t) * 8 + (ev)] = __builtin_amdgcn_s_memrealtime()
  // granules per row: bf16 h → H/2 (2 units each), F32 h → H (one unit each)
  constexpr int GPR = F32 ? H : H / 2;
  unsigned long long* xg = xg_all + (size_t)team * 2 * Bc * GPR;

  // zero the padding rows of both h buffers once
  if constexpr (!V1)
    for (int i = tid; i < 2 * RB * HP; i += NT) (&hl[0][0][0])[i] = 0;
  if constexpr (F32 && !V1)
    for (int i = tid; i < 2 * RB * HP; i += NT) (&hlo[0][0][0])[i] = 0;

  // W_hh slice for this wave's tile: columns c = 4·ul + q ↔ gate row q·H + j0 + 4·wv + ul, full K, in VGPRs
  // (F32: fp32 W_hh split into hi/lo bf16 fragments once, here)
  const bool mfma_wave = wv < NTILE;
  const int col = lane & 15, kg = lane >> 4;
  bf16x8 wf[V1 ? 1 : KSTEP];
  bf16x8 wfl[F32 && !V1 ? KSTEP : 1];
  float wq[V1 ? 4 * KSL : 1];
  if (mfma_wave) {
    const int row = (col & 3) * H + j0 + 4 * wv + (col >> 2);
    if constexpr (V1) {
      // lane (u = lane/LPU, slice = lane%LPU): W_hh rows of the 4 gates of unit j0 + UPW·wv + u over the slice
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float* wr = static_cast<const float*>(whh_) + (size_t)(g * H + j0 + UPW * wv + lane / LPU) * H +
                          (lane % LPU) * KSL;
#pragma unroll
        for (int j = 0; j < KSL; j += 4) {
          const float4 v = *reinterpret_cast<const float4*>(wr + j);
          wq[g * KSL + j] = v.x; wq[g * KSL + j + 1] = v.y; wq[g * KSL + j + 2] = v.z; wq[g * KSL + j + 3] = v.w;
        }
      }
    } else if constexpr (F32) {
      const float* whh = static_cast<const float*>(whh_);
#pragma unroll
      for (int ks = 0; ks < KSTEP; ++ks) split_frag(whh + (size_t)row * H + ks * 32 + 8 * kg, wf[ks], wfl[ks]);
    } else {
      const short* whh = static_cast<const short*>(whh_);
#pragma unroll
      for (int ks = 0; ks < KSTEP; ++ks)
        wf[ks] = *reinterpret_cast<const bf16x8*>(whh + (size_t)row * H + ks * 32 + 8 * kg);
    }
  }
  // elementwise mapping after the 4×4 transpose: lane → (row 4·kg + (col&3) [+16·mt], unit j0 + 4·wv + col/4)
  // (V1: lane (u, slice) → row = slice — only slice 0 is a live row —, unit j0 + 4·wv + u)
  const int erow = V1 ? (lane % LPU) : 4 * kg + (col & 3);
  const int eunit = j0 + (V1 ? UPW * wv + lane / LPU : 4 * wv + (col >> 2));
  // folded LSTM bias (b_ih + b_hh, unit-major): xp4 may then be the bare input projection
  const dca::f32x4 bv = (bias4 && mfma_wave) ? *reinterpret_cast<const dca::f32x4*>(bias4 + eunit * 4)
                                             : dca::f32x4{0.f, 0.f, 0.f, 0.f};

  // V1 merged outputs: every lane of a unit's LPU-lane group carries every row's state (the dot products are
  // summed into all of them anyway), so c and h leave in ONE store instruction — slice-2r lanes write row r's c,
  // slice-(2r+1) lanes its h — and a step queues two output stores (c|h, gates) behind its publish instead of three
  // (cs, hsf, gates): the stores ahead of the next poll are what the step pays for (profiles/deferred_output_stores.md).
  // Measured (scripts/team_store_ab.py, bench A/B on one box): 1.420 vs 1.447 µs per standalone forward step,
  // 4.874 vs 4.945 ms per learner step.
  const int slice = V1 ? lane % LPU : 0;
  unsigned spins = 0;
  unsigned long long since = 0;
  for (unsigned iter = 0;; ++iter) {
    const int chain = next_chain(ctl, team, m, iter, nch, &sh_int);
    if (chain < 0) break;
    const int b0 = chain * Bc;
    const int B = min(Bc, Btot - b0);
    const unsigned tagbase = make_tagbase(epoch, iter);
    float creg[NR], hreg[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int b = V1 ? i : i * 16 + erow;
      creg[i] = (mfma_wave && b < B) ? c0[(size_t)(b0 + b) * H + eunit] : 0.f;
      hreg[i] = 0.f;
    }
    // Land the chain-start loads here, once per chain (the technique of lstm_team_bwd.hip, ccv): left pending into the
    // step loop, the compiler's wait-count merge at the loop header takes creg for a load in flight in EVERY
    // iteration — a vmcnt(0) ahead of the product (read of the loop-carried copy) and one at the back edge (write
    // into it), the second behind the publish and the output stores, so that every wave waited out their
    // acknowledgement before it issued the next step's prefetch and first poll. The bias vector is loaded once per
    // launch and read in every step in the same way. Hazards: profiles/recurrence_fwd_waits.md.
#pragma unroll
    for (int i = 0; i < NR; ++i) asm volatile("" ::"v"(creg[i]));
    asm volatile("" ::"v"(bv));
    bool dead = false;
    for (int t = 0; t < S; ++t) {
      const int par = t & 1;
      spins = 0;
      since = 0;
      TSTAMP(0);
      // ---- prefetch this step's input projection (one 16-B vector per owned (row, unit)). Loading it one step
      // ahead instead measured slower (2.11 vs 1.94 µs per step at B=8, H=512).
      dca::f32x4 xv[NR];
      // sequence packing: an episode starts at step t (h, c := 0). The flag byte is kept raw and compared only at its
      // use, after the gather: a compare here (the old `rst[..] != 0` bool) waited out the load before the gather
      // started — measured +0.29 ms per B=8, S=1400 call for passing any reset tensor, zeros included.
      int rzb[NR];
      if (mfma_wave) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int b = V1 ? i : i * 16 + erow;         // (V1: the group's lanes load the same 16 B, one request)
          const size_t tx = ((knobs >> 10) & 1) ? 0 : (size_t)t;   // knob: every step reads step 0 (L2-resident)
          xv[i] = (b < B) ? *reinterpret_cast<const dca::f32x4*>(xp4 + (((size_t)(b0 + b) * sb + tx * st) * H + eunit) * 4)
                          : dca::f32x4{0.f, 0.f, 0.f, 0.f};
          rzb[i] = 0;
          if (rst != nullptr)                           // (uniform; rows >= B read sequence 0's flag and are never
            rzb[i] = rst[(size_t)(b < B ? b0 + b : 0) * sb + (size_t)t * st];   // stored. Not b0's: the plan's last
                                                        // chain may be empty, b0 ≥ Btot, and its flag past the end)
        }
      } else {
#pragma unroll
        for (int i = 0; i < NR; ++i) {                  // (defined in every wave: all of them land it below)
          xv[i] = dca::f32x4{0.f, 0.f, 0.f, 0.f};
          rzb[i] = 0;
        }
      }
      // ---- gather h_{t-1} into hl[par]
      if (t == 0) {
        for (int i = tid; i < B * H; i += NT) {
          const int b = i / H, k = i % H;
          const float v = h0[(size_t)(b0 + b) * H + k];
          if constexpr (V1) {
            hf[par][b * ROWF + (k / KSL) * SP + k % KSL] = v;
          } else {
            hl[par][b][k] = dca::f2bf(v);
            if constexpr (F32) hlo[par][b][k] = dca::f2bf(v - dca::bf2f(dca::f2bf(v)));
          }
        }
      } else {
        const unsigned tag = tagbase | (unsigned)t;          // h_{t-1} carries tag t
        const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(xg + (size_t)((t - 1) & 1) * Bc * GPR, Bc * GPR * 8);
        constexpr int CPR = F32 ? H / 2 : H / 4;              // 16-B chunks (2 f32 / 4 bf16 h values) per row
        constexpr int NL = ((V1 ? R : RB) * CPR + NT - 1) / NT;   // (V1: R rows)
        // every chunk is re-polled only until it has arrived, so later rounds move only the missing bytes
        i32x4 g[NL];
        bool okc[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) okc[i] = tid + NT * i >= B * CPR;
        for (int i = 0; i < (knobs & 0xff); ++i) __builtin_amdgcn_s_sleep(1);
        if ((knobs >> 9) & 1) {
          while (!okc[0]) {
            g[0] = __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, 0, kSc1);
            okc[0] = ((unsigned)g[0].y == tag) & ((unsigned)g[0].w == tag);
            if (__all(okc[0])) break;
            if (spin_fail(spins, since, ctl, err, 1u, knobs)) { dead = true; break; }
          }
        }
        while (!dead) {
#pragma unroll
          for (int i = 0; i < NL; ++i)
            if (!okc[i]) g[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + NT * i) * 16, 0, kSc1);
          bool ok = true;
#pragma unroll
          for (int i = 0; i < NL; ++i) {
            okc[i] = okc[i] || (((unsigned)g[i].y == tag) & ((unsigned)g[i].w == tag));
            ok &= okc[i];
          }
          if (__all(ok)) break;
          if (spin_fail(spins, since, ctl, err, 1u, knobs)) { dead = true; break; }
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const int ci = tid + NT * i;
          if (ci < B * CPR) {
            if constexpr (V1) {
              const int b = ci / CPR, k = 2 * (ci % CPR);
              *reinterpret_cast<float2*>(&hf[par][b * ROWF + (k / KSL) * SP + k % KSL]) =
                  make_float2(__int_as_float(g[i].x), __int_as_float(g[i].z));
            } else if constexpr (F32) {
              const int b = ci / CPR, k = (ci % CPR) * 2;
              const float x = __int_as_float(g[i].x), z = __int_as_float(g[i].z);
              const short xh = dca::f2bf(x), zh = dca::f2bf(z);
              *reinterpret_cast<unsigned*>(&hl[par][b][k]) = (unsigned)(unsigned short)xh | ((unsigned)(unsigned short)zh << 16);
              *reinterpret_cast<unsigned*>(&hlo[par][b][k]) =
                  (unsigned)(unsigned short)dca::f2bf(x - dca::bf2f(xh)) |
                  ((unsigned)(unsigned short)dca::f2bf(z - dca::bf2f(zh)) << 16);
            } else {
              const int b = ci / CPR, k = (ci % CPR) * 4;
              *reinterpret_cast<u32x2*>(&hl[par][b][k]) = u32x2{(unsigned)g[i].x, (unsigned)g[i].z};
            }
          }
        }
      }
      // Land the step's prefetch (xv, the reset byte) here, behind the gather. At t > 0 a polling wave has just waited
      // vmcnt(0) for its last poll round and returns are in order, so this wait finds nothing outstanding; at t = 0
      // and in a wave with no chunk to poll it is the wait the step needs anyway. Without it the compiler carries
      // "xv / rzb may be in flight" round the back edge (the paths with no poll have no wait) and protects next step's
      // writes into these registers at the top of the step: vmcnt(1) behind the xv prefetch when no reset tensor is
      // passed, which drains the publish and the output stores ahead of the first poll exactly as the back-edge wait
      // did. In every wave and outside any branch: a path round it would keep the registers "in flight".
#pragma unroll
      for (int i = 0; i < NR; ++i) asm volatile("" ::"v"(xv[i]), "v"(rzb[i]));
      TSTAMP(1);
      if (dead) sh_int = -2;
      lds_barrier();
      if (sh_int == -2) break;
      TSTAMP(2);
      if constexpr (V1) {
       // (only the waves that own units: at H < 512 a workgroup's U = H/32 units take U/4 of its 4 waves — the
       // others have no W_hh slice and would publish / store other workgroups' units)
       if (mfma_wave) {
        // ---- exact fp32 VALU, R rows: the 4 gates of this lane's unit over its K slice for every row (W_hh slice in
        // VGPRs reused across the rows), summed over the unit's LPU slices — every lane of the group holds every row
        float hpub = 0.f;
        [[maybe_unused]] float ocv = 0.f, ohv = 0.f;
        [[maybe_unused]] dca::f32x4 oav = {0.f, 0.f, 0.f, 0.f};
        if constexpr (R == 8) {
          // 8 rows: one row at a time from the dot products to the select of what this lane stores, so that no
          // per-row array (pre-activations, activations, c, h: 10 values × 8 rows) is live beside the W_hh slice
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (r < B) {                                      // (B is uniform)
              float g0, g1, g2, g3;
              pk_dot4<KSL>(wq, &hf[par][r * ROWF + slice * SP], g0, g1, g2, g3);
              g0 = row_sum16(g0); g1 = row_sum16(g1); g2 = row_sum16(g2); g3 = row_sum16(g3);
              if (rzb[r]) { g0 = 0.f; g1 = 0.f; g2 = 0.f; g3 = 0.f; }   // episode start
              const float pi = g0 + (xv[r][0] + bv[0]), pf = g1 + (xv[r][1] + bv[1]),
                          pg = g2 + (xv[r][2] + bv[2]), po = g3 + (xv[r][3] + bv[3]);
              const float ig = sigm<PREC>(pi), fg = sigm<PREC>(pf), gg = tanh_<PREC>(pg), og = sigm<PREC>(po);
              const float c = fg * (rzb[r] ? 0.f : creg[r]) + ig * gg;
              const float hv = og * tanh_<PREC>(c);
              creg[r] = c; hreg[r] = hv;
              if (slice == r) hpub = hv;
              if ((slice >> 1) == r) { ocv = c; ohv = hv; oav = dca::f32x4{ig, fg, gg, og}; }
            }
          }
        }
        float g[R == 8 ? 1 : R][4];
#pragma unroll
        for (int r = 0; r < (R == 8 ? 0 : R); ++r) {
          if (r < B) {                                        // (B is uniform)
            pk_dot4<KSL>(wq, &hf[par][r * ROWF + slice * SP], g[r][0], g[r][1], g[r][2], g[r][3]);
            // (Tried, one row: a reduce-SCATTER over the 16 slices — xor 1 / xor 2 quad swaps then row_ror 4 / 8, 4
            // DPP moves instead of 16 — with one activation per lane and a quad broadcast of the four gates: 1.500 vs
            // 1.481 µs per standalone step, no gain in the learner step; the plain row sums stay.)
#pragma unroll
            for (int q = 0; q < 4; ++q) g[r][q] = row_sum16(g[r][q]);
          }
        }
        float act[R == 8 ? 1 : R][4], cr[R == 8 ? 1 : R], hr[R == 8 ? 1 : R];
#pragma unroll
        for (int r = 0; r < (R == 8 ? 0 : R); ++r) {
          cr[r] = hr[r] = 0.f;
          act[r][0] = act[r][1] = act[r][2] = act[r][3] = 0.f;
          if (r < B) {
            if (rzb[r]) { g[r][0] = 0.f; g[r][1] = 0.f; g[r][2] = 0.f; g[r][3] = 0.f; }   // episode start
            const float pi = g[r][0] + (xv[r][0] + bv[0]), pf = g[r][1] + (xv[r][1] + bv[1]),
                        pg = g[r][2] + (xv[r][2] + bv[2]), po = g[r][3] + (xv[r][3] + bv[3]);
            const float ig = sigm<PREC>(pi), fg = sigm<PREC>(pf), gg = tanh_<PREC>(pg), og = sigm<PREC>(po);
            const float c = fg * (rzb[r] ? 0.f : creg[r]) + ig * gg;
            const float hv = og * tanh_<PREC>(c);
            creg[r] = c; hreg[r] = hv; cr[r] = c; hr[r] = hv;
            act[r][0] = ig; act[r][1] = fg; act[r][2] = gg; act[r][3] = og;
            if (slice == r) hpub = hv;
          }
        }
        TSTAMP(3);
        // ---- publish h_t: the slice-r lane of every unit group publishes row r's granule {f32 h(u), tag}
        if (slice < B) {
          const u32x2 gv = {(unsigned)__float_as_int(hpub), tagbase | (unsigned)(t + 1)};
          const __amdgpu_buffer_rsrc_t ws = uniform_rsrc(xg + (size_t)par * Bc * GPR, Bc * GPR * 8);
          __builtin_amdgcn_raw_buffer_store_b64(gv, ws, (slice * H + eunit) * 8, 0, kPlain);
        }
        TSTAMP(4);
        // ---- outputs, one store instruction per lane: slice 2r → row r's c (+ its gates), slice 2r+1 → row r's h
        // (one b32 store for everything — slices 0-3 the gates, 4 c, 5 h — measured slower: 1.476 vs 1.410 µs)
        const int orow = slice >> 1;
        if (orow < B && orow < R && !((knobs >> 8) & 1)) {
          float cv = 0.f, hv = 0.f;
          dca::f32x4 av = {0.f, 0.f, 0.f, 0.f};
          if constexpr (R == 8) { cv = ocv; hv = ohv; av = oav; }
#pragma unroll
          for (int r = 0; r < (R == 8 ? 0 : R); ++r)
            if (orow == r) { cv = cr[r]; hv = hr[r]; av = dca::f32x4{act[r][0], act[r][1], act[r][2], act[r][3]}; }
          const size_t o = ((size_t)(b0 + orow) * sb + (size_t)t * st) * H + eunit;
          gstore((slice & 1) ? hsf + o : cs + o, (slice & 1) ? hv : cv);
          if (!(slice & 1)) *reinterpret_cast<dca::f32x4*>(gates4 + o * 4) = av;
        }
        TSTAMP(5);
       }
      } else if (mfma_wave) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (mt * 16 >= B) break;                            // wave-uniform
          float gq0 = 0.f, gq1 = 0.f, gq2 = 0.f, gq3 = 0.f;
          {
          // ---- gates pre-activation tile: rows = batch, columns = (unit, gate)
          dca::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if constexpr (F32) {
            // three independent accumulation chains (hi·hi, lo·hi, hi·lo) keep the MFMA pipe full
            dca::f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEP; ++ks) {
              const bf16x8 a = *reinterpret_cast<const bf16x8*>(&hl[par][mt * 16 + col][ks * 32 + 8 * kg]);
              const bf16x8 al = *reinterpret_cast<const bf16x8*>(&hlo[par][mt * 16 + col][ks * 32 + 8 * kg]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ks], acc, 0, 0, 0);
              a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[ks], a1, 0, 0, 0);
              a2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wfl[ks], a2, 0, 0, 0);
            }
            acc += a1 + a2;
          } else {
#pragma unroll
            for (int ks = 0; ks < KSTEP; ++ks) {
              const bf16x8 a = *reinterpret_cast<const bf16x8*>(&hl[par][mt * 16 + col][ks * 32 + 8 * kg]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ks], acc, 0, 0, 0);
            }
          }
          // ---- 4×4 transpose inside each group of 4 lanes: lane (q' = col&3) gets gate q of row 4kg+q'. Round j:
          // lane a sends its value for row (a-j)&3 and receives from lane (a+j)&3 of its quad — a DPP quad_perm
          // (register-to-register, a few cycles) instead of an LDS-routed ds_bpermute
          const int q0 = col & 3;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int sel = (q0 - j) & 3;                       // what this lane sends in round j
            const float send = sel == 0 ? acc[0] : sel == 1 ? acc[1] : sel == 2 ? acc[2] : acc[3];
            const int qs = (q0 + j) & 3;                        // gate carried by the received value
            // quad_perm [(0+j)&3, (1+j)&3, (2+j)&3, (3+j)&3]: 0xE4 (identity), 0x39, 0x4E, 0x93
            float got = send;
            if (j == 1) got = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0x39, 0xF, 0xF, false));
            if (j == 2) got = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0x4E, 0xF, 0xF, false));
            if (j == 3) got = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0x93, 0xF, 0xF, false));
            gq0 = qs == 0 ? got : gq0;
            gq1 = qs == 1 ? got : gq1;
            gq2 = qs == 2 ? got : gq2;
            gq3 = qs == 3 ? got : gq3;
          }
          }
          const int b = mt * 16 + erow;
          if (rzb[mt]) { gq0 = 0.f; gq1 = 0.f; gq2 = 0.f; gq3 = 0.f; }   // episode start: no recurrent term
          // (bias added here, at the use: an add right after the prefetch would wait out the load before the gather)
          const float pi = gq0 + (xv[mt][0] + bv[0]), pf = gq1 + (xv[mt][1] + bv[1]), pg = gq2 + (xv[mt][2] + bv[2]),
                      po = gq3 + (xv[mt][3] + bv[3]);
          const float ig = sigm<PREC>(pi), fg = sigm<PREC>(pf), gg = tanh_<PREC>(pg), og = sigm<PREC>(po);
          const float c = fg * (rzb[mt] ? 0.f : creg[mt]) + ig * gg;
          const float hv = og * tanh_<PREC>(c);
          if (b < B) { creg[mt] = c; hreg[mt] = hv; }
          TSTAMP(3);
          if constexpr (F32) {
            // ---- publish h_t: granule {f32 h(u), tag} by every lane of a live row
            if (b < B) {
              const u32x2 gv = {(unsigned)__float_as_int(hv), tagbase | (unsigned)(t + 1)};
              const __amdgpu_buffer_rsrc_t ws = uniform_rsrc(xg + (size_t)par * Bc * GPR, Bc * GPR * 8);
              __builtin_amdgcn_raw_buffer_store_b64(gv, ws, (b * H + eunit) * 8, 0, kPlain);
            }
          } else {
            // ---- publish h_t: granule {h(u), h(u+1)} by the even-unit lane (partner unit is 4 lanes up)
            // partner unit's h from 4 lanes up, same 16-lane row: DPP row_shl:4 (register-to-register)
            const float hnb = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(hv), 0x104, 0xF, 0xF, false));
            if (b < B && ((col >> 2) & 1) == 0) {
              const unsigned pl = (unsigned)(unsigned short)dca::f2bf(hv) | ((unsigned)(unsigned short)dca::f2bf(hnb) << 16);
              const u32x2 gv = {pl, tagbase | (unsigned)(t + 1)};
              const __amdgpu_buffer_rsrc_t ws = uniform_rsrc(xg + (size_t)par * Bc * GPR, Bc * GPR * 8);
              __builtin_amdgcn_raw_buffer_store_b64(gv, ws, (b * (H / 2) + (eunit >> 1)) * 8, 0, kPlain);
            }
          }
          TSTAMP(4);
          // ---- outputs
          if (b < B && !((knobs >> 8) & 1)) {
            const size_t bt = (size_t)(b0 + b) * sb + (size_t)t * st;
            if (hs) hs[bt * H + eunit] = dca::f2bf(hv);
            if (hsf) hsf[bt * H + eunit] = hv;
            cs[bt * H + eunit] = c;
            *reinterpret_cast<dca::f32x4*>(gates4 + (bt * H + eunit) * 4) = dca::f32x4{ig, fg, gg, og};
          }
          TSTAMP(5);
        }
      }
      // Back edge: no wait on vector memory here (the compiler used to place vmcnt(0), see the landing of creg above).
      // The publish and the output stores of step t are still in flight when step t + 1 issues its prefetch and its
      // first poll. Nothing relied on that drain:
      // * hand-off: a granule carries data and tag in ONE 8-byte store, so a consumer that sees tag t + 1 sees h_t;
      //   no later store of this wave completes or orders it.
      // * slot reuse: the parity slot of step t is written again at t + 2. A wave gets there only behind its gather of
      //   step t + 2, i.e. after EVERY workgroup published t + 1, which each did behind its own gather of t + 1 — its
      //   last read of slot t. Program order per wave plus the tags, not vmcnt.
      // * outputs (h / c / gates, hn / cn): never read back by this kernel; the launch's end makes them visible.
      //   xv and the reset byte are read-only inputs. Registers: a store reads its data when it issues.
      // * vmcnt returns are in order, so step t + 1's poll wait still covers these stores; what is gone is waiting for
      //   them BEFORE the poll is issued.
      // * the dead → sh_int = -2 → break hand-shake runs on LDS and the barrier; the chain-end stores (hn, cn, the
      //   `done` counter behind __syncthreads) and next_chain's control-block loads keep their own waits.
    }
#undef TSTAMP
    if (sh_int == -2) return;
    if (mfma_wave) {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int b = V1 ? i : i * 16 + erow;
        if (b < B && (!V1 || slice == i)) {
          hn[(size_t)(b0 + b) * H + eunit] = hreg[i];
          cn[(size_t)(b0 + b) * H + eunit] = creg[i];
        }
      }
    }
    __syncthreads();
    if (tid == 0) add_agent(&ctl->done[team], 1u);
  }
}

template <Prod P, int ROWS, int KS, bool LIBM>
__global__ __launch_bounds__(form_threads(P), 1) void lstm_team_fwd_kernel(
    const float* __restrict__ xp4, const void* __restrict__ whh, const float* __restrict__ h0,
    const float* __restrict__ c0, short* __restrict__ hs, float* __restrict__ hsf, float* __restrict__ cs,
    float* __restrict__ gates4, float* __restrict__ hn, float* __restrict__ cn, unsigned long long* xg_all,
    TeamCtl* ctl, unsigned* err, int Btot, int Bc, int nch, int S, int sb, int st, unsigned long long* trace,
    int knobs, const float* __restrict__ bias4, const unsigned char* __restrict__ rst) {
  __builtin_amdgcn_s_setprio(3);   // issue priority over co-resident waves of kernels overlapped on other streams
  lstm_team_fwd_body<P, ROWS, KS, LIBM>(xp4, whh, h0, c0, hs, hsf, cs, gates4, hn, cn, xg_all, ctl, err, Btot, Bc, nch, S, sb,
                             st, trace, knobs, bias4, rst);
  team_exit(ctl, err, nch);
}

}  // namespace

// Bytes of the control block (TeamCtl, caller-owned, one per stream).
extern "C" size_t dca_lstm_team_ctl_bytes() { return 256; }

// Sequence chains a launch of B sequences is split into (rows of the backward's bias-gradient partials).
// -1: not a plan (bad `rows`, `rows` without `exact`, `exact` without fp32 weights, more chains than kMaxQueue).
extern "C" int dca_lstm_team_chains(int B, int f32, int exact, int rows) {
  int nch, Bc, MT;
  if (!plan_any(B, f32, exact, rows, nch, Bc, MT)) return -1;
  return nch;
}

// Exchange-buffer bytes (per-team hand-off rings) for a launch of (B, H). Not zeroed: tags carry the epoch.
extern "C" size_t dca_lstm_team_workspace(int B, int H, int backward, int f32, int exact, int rows) {
  int nch, Bc, MT;
  if (!plan_any(B, f32, exact, rows, nch, Bc, MT)) return 0;
  if (!backward) return (size_t)kMaxTeams * 2 * Bc * (f32 ? H : H / 2) * 8;
  return (size_t)kMaxTeams * 2 * Bc * H * (f32 ? 2 : 1) * 16;
}

// whh: (4H,H) bf16 (f32 = 0) or fp32 (f32 = 1: h exchanged and stored in fp32, hs unused). The kernel: select_form.
extern "C" hipError_t dca_lstm_team_fwd(const float* xp4, const void* whh, const float* h0, const float* c0,
                                        short* hs, float* hsf, float* cs, float* gates4, float* hn, float* cn,
                                        void* ctl_mem, void* ws, size_t ws_bytes, unsigned* err, int B, int S, int H,
                                        int time_major, hipStream_t stream, unsigned long long* trace,
                                        const float* bias4, int f32, int precise, const unsigned char* rst,
                                        int exact, int rows) {
  if (B < 1 || S < 1 || S >= 65535 || (H != 128 && H != 256 && H != 512)) return hipErrorInvalidValue;
  int nch, Bc, MT;
  if (!plan_any(B, f32, exact, rows, nch, Bc, MT)) return hipErrorInvalidValue;
  if (ws_bytes < dca_lstm_team_workspace(B, H, 0, f32, exact, rows) || ctl_mem == nullptr) return hipErrorInvalidValue;
  if (f32 && hsf == nullptr) return hipErrorInvalidValue;
  if (!f32 && hs == nullptr) return hipErrorInvalidValue;
  const int sb = time_major ? 1 : S, st = time_major ? B : 1;   // row(b, t) = b·sb + t·st
  TeamCtl* ctl = reinterpret_cast<TeamCtl*>(ctl_mem);
  unsigned long long* xg = reinterpret_cast<unsigned long long*>(ws);
  const Form form = select_form(f32 != 0, Bc, H, false, precise != 0, exact != 0);
#define DCA_F(P, ROWS, H_, LIBM)                                                                                \
  if (form == Form{Prod::P, ROWS, H_, LIBM}) {                                                                  \
    lstm_team_fwd_kernel<Prod::P, ROWS, H_ / 128, LIBM><<<kMaxTeams * kT, form_threads(Prod::P), 0, stream>>>(  \
        xp4, whh, h0, c0, hs, hsf, cs, gates4, hn, cn, xg, ctl, err, B, Bc, nch, S, sb, st, trace, team_knobs(), \
        bias4, rst);                                                                                            \
    return hipGetLastError();                                                                                   \
  }
  DCA_TEAM_FWD_FORMS(DCA_F)
#undef DCA_F
  return hipErrorInvalidValue;           // kNoForm
}
