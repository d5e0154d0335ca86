// XCD-team persistent LSTM recurrence for gfx950 — the default learner recurrence. What the forward
// (lstm_team_fwd.hip) and the backward (lstm_team_bwd.hip) share: the team protocol, the exact-VALU dot product, the
// launch plan, and the one table that says which kernel form a launch runs (select_form, at the end).
//
// The mapping. A recurrence step is latency-bound: its critical path is one all-to-all hand-off of the step's state
// between the workgroups that own slices of W_hh. A TEAM of 32 workgroups — one per CU of a single XCD — runs a whole
// sequence chain and exchanges through that XCD's shared L2: plain stores keep the lines in L2 and sc1 polls (L1
// bypass, L2-served) see them ≈0.2 µs later (scripts/ubench/xcd_pingpong.hip: 451 ns round trip same-XCD vs 768 ns
// cross-XCD, idle). Up to 8 teams (one per XCD) run independent chains of ≤ 32 sequences concurrently. Each workgroup
// (member m of 32) owns U = H/32 hidden units J_m = [mU, mU+U) and their 4U gate rows of W_hh, kept in registers for
// the whole launch. The fp32-exact learner's launches (`exact`, plan_exact) stay on the exact fp32 VALU forms at every
// batch size: chains of 1, 2, 4 or 8 rows, one per team up to 64 sequences, queued chains of 8 rows beyond, 32 chains
// at the most (kMaxQueue, at make_tagbase) = 256 sequences per launch.
//
// Team formation is placement-robust: every workgroup reads HW_REG_XCC_ID and takes a ticket on its XCC's
// counter; the first 32 of an XCC form its team, a leader commits the team only when all 32 arrived (bounded
// wait), and committed teams pull chains from a shared queue — so any dispatch that lands ≥ 32 workgroups on at
// least one XCD finishes every chain. An XCD whose team cannot form is not an error by itself (the other teams
// drain the queue); only chains left UNPROCESSED are: the last workgroup to exit checks the queue and sets
// *err = 3. Error codes (1 forward hand-off timeout, 2 backward timeout, 3 unprocessed chains) are sticky; the
// learner reduces the flag across DP ranks with the has-grad counts and the fused Adam skips the update when it
// is set (learner/engine.py), so a failed recurrence never reaches the weights; FusedPolicy.check_error raises at
// the iteration boundary (before checkpoint / publish). DCA_TEAM_FAIL=1 makes every workgroup refuse to form a
// team (fault-injection tests).
//
// Layouts (unit-major gates "(H,4)" so a hidden unit's 4 gates are one 16-byte vector):
//   xp4    (B, S, H, 4) f32  x·W_ihᵀ + b_ih + b_hh with W_ih rows permuted to (unit, gate) order
//   whh    (4H, H)      bf16 or f32, PyTorch layout (gate-major rows i,f,g,o)
//   gates4 (B, S, H, 4) f32  activated i, f, g, o          dgates4 (B, S, H, 4) f32 ∂L/∂pre-activations
//   hs (B,S,H) bf16, hsf (B,S,H) f32 (optional), cs (B,S,H) f32, h0/c0/hn/cn/dh0/dc0 (B,H) f32
// (time-major launches: (S, B, …); the kernels address row (b, t) as b·sb + t·st).
//
// Measurements behind the design, and what was tried and left out: profiles/deferred_output_stores.md (output store
// placement and deferral), profiles/recurrence_wave_gather.md (wave-private gather, lazy deadline stamp),
// profiles/recurrence_bwd_handoff.md (∂h hand-off), profiles/exact_big_batch.md (8-row chains, the exact plan beyond
// 32 sequences), profiles/recurrence_left_out.md (role-separated forward, ring forward, double-buffered poll, packed
// record), profiles/recurrence_forms.md (the kernel forms and their resource figures).
#pragma once
#include "common.h"
#include <cstdlib>

namespace {

using dca::bf16x8;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kT = 32;                  // workgroups per team (CUs per XCD)
constexpr int kMaxTeams = 8;
constexpr int kThreads = 256;
constexpr int kSc1 = 16;                // buffer cache policy: sc1 (bypass the CU's L1, served by the XCD L2)
constexpr int kPlain = 0;               // plain store: write-through L1, line stays in the XCD L2

// Persistent control block (one per stream, zero-initialised once, caller-owned). It is SELF-CLEANING: the last
// workgroup of a launch to exit resets every field and bumps ``epoch``, so a launch never depends on a memset —
// which also makes the kernels safe to replay from a hipGraph. ``epoch`` is folded into every hand-off tag, so
// exchange buffers need no zeroing either: data left by an earlier launch can never match.
struct TeamCtl {
  unsigned xcnt[16];                     // tickets per XCC
  unsigned state[kMaxTeams];             // 0 pending, 1 committed, 2 aborted
  unsigned chain[kMaxTeams];             // (announce iter << 16) | chain id
  unsigned done[kMaxTeams];              // members that finished their current chain
  unsigned next_chain;
  unsigned abort;
  unsigned exits;                        // workgroups that have left the launch
  unsigned epoch;                        // launches completed on this control block
};
static_assert(sizeof(TeamCtl) <= 256, "TeamCtl must fit the 256-byte control tensor");

__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf; }
__device__ __forceinline__ unsigned ld_acq(const unsigned* p) {
  return __hip_atomic_load((__attribute__((address_space(1))) unsigned*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_rel(unsigned* p, unsigned v) {
  __hip_atomic_store((__attribute__((address_space(1))) unsigned*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned add_agent(unsigned* p, unsigned v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// explicit global (not flat) stores for the per-lane-address merged stores: a flat store would also count in lgkmcnt,
// which the LDS barriers wait on
template <typename T>
__device__ __forceinline__ void gstore(T* p, T v) { *(__attribute__((address_space(1))) T*)p = v; }
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- V1 (exact fp32 VALU) dot products. Lane (r = lane/16, s = lane%16) of a wave owns FOUR outputs (the 4 gates
// of one unit forward, 4 units backward) over ONE K slice of KSL = K/16 elements: the slice's operand is read from LDS
// once (KSL/4 ds_read_b128, shared by the 4 rows through the LDS broadcast) and feeds 4 outputs, then a DPP row
// reduction sums the 16 slices. The step is bound by LDS return bandwidth and VALU issue, not by the FMAs: the first
// layout (lane = one output over a K quarter) read 4× the bytes — 32 × 1 KB per wave per step, 0.64 µs of compute
// phase at H = 512 — and a register/DPP-broadcast operand (one v_mov_dpp per FMA) was slower still (0.84 µs). FMAs
// issue as packed fp32 (v_pk_fma_f32, two outputs per instruction), two chains (even / odd k) per output pair.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int KSL>
__device__ __forceinline__ void pk_dot4(const float* wq, const float* x, float& o0, float& o1, float& o2, float& o3) {
  f32x2 a01e = {0.f, 0.f}, a01o = {0.f, 0.f}, a23e = {0.f, 0.f}, a23o = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < KSL; j += 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j);
    a01e = __builtin_elementwise_fma(f32x2{wq[j], wq[KSL + j]}, f32x2{v.x, v.x}, a01e);
    a23e = __builtin_elementwise_fma(f32x2{wq[2 * KSL + j], wq[3 * KSL + j]}, f32x2{v.x, v.x}, a23e);
    a01o = __builtin_elementwise_fma(f32x2{wq[j + 1], wq[KSL + j + 1]}, f32x2{v.y, v.y}, a01o);
    a23o = __builtin_elementwise_fma(f32x2{wq[2 * KSL + j + 1], wq[3 * KSL + j + 1]}, f32x2{v.y, v.y}, a23o);
    a01e = __builtin_elementwise_fma(f32x2{wq[j + 2], wq[KSL + j + 2]}, f32x2{v.z, v.z}, a01e);
    a23e = __builtin_elementwise_fma(f32x2{wq[2 * KSL + j + 2], wq[3 * KSL + j + 2]}, f32x2{v.z, v.z}, a23e);
    a01o = __builtin_elementwise_fma(f32x2{wq[j + 3], wq[KSL + j + 3]}, f32x2{v.w, v.w}, a01o);
    a23o = __builtin_elementwise_fma(f32x2{wq[2 * KSL + j + 3], wq[3 * KSL + j + 3]}, f32x2{v.w, v.w}, a23o);
  }
  const f32x2 a01 = a01e + a01o, a23 = a23e + a23o;
  o0 = a01.x; o1 = a01.y; o2 = a23.x; o3 = a23.y;
}
// Σ over the 16 lanes of this lane's DPP row, result in every lane: xor 1, xor 2 (quad_perm), half-row and row mirrors
__device__ __forceinline__ float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

// activations: the fast forms (v_exp_f32 + v_rcp_f32, ≈1e-7 relative) or, in the fp32-exact learner, libm expf /
// tanhf with IEEE division
template <bool PREC>
__device__ __forceinline__ float sigm(float x) { return PREC ? 1.f / (1.f + expf(-x)) : dca::sigmoidf_(x); }
template <bool PREC>
__device__ __forceinline__ float tanh_(float x) { return PREC ? tanhf(x) : dca::tanhf_(x); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* p, int bytes) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), (short)0,
                                           __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// Bounded spin bookkeeping; true when this wave must give up (timeout or another workgroup raised an error). The
// limit is WALL-CLOCK per wait (s_memrealtime, 100 MHz): ≈2 s without one hand-off arriving (DCA_TEAM_PATIENT: ≈60 s,
// for runs that share the GPU with another process's kernels). It used to count polls over the whole launch, so a
// recurrence slowed by co-resident kernels (the node loop's actor graph replays) could trip it with no hand-off ever
// lost — the cumulative count grows with every step's extra polls (the config-5 loop's one backward timeout, code 2).
// `spins` restarts at every step (the back-off sleep after 32 polls: within ±0.01 µs of never sleeping), and `since`
// restarts with it as 0 = "not stamped yet". The clock is first read at the wait's 256th failed poll (≈0.1 ms in,
// nothing against the limit), never between a step's first failed poll and its second: stamping at the first
// failure put a scalar-memory round trip (s_memrealtime + s_waitcnt lgkmcnt(0)) ahead of the second poll round of
// nearly every step of both kernels.
__device__ __forceinline__ bool spin_fail(unsigned& spins, unsigned long long& since, TeamCtl* ctl, unsigned* err,
                                          unsigned code, int knobs) {
  asm volatile("" ::: "memory");        // compiler barrier: re-issue the poll loads every round
  ++spins;
  if ((spins & 255u) == 0) {
    if (ld_acq(&ctl->abort) != 0) return true;
    const unsigned long long limit = ((knobs >> 15) & 1) ? 6000000000ull : 200000000ull;
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    if (since == 0) {
      since = now;
    } else if (now - since > limit) {
      st_rel(err, code);
      st_rel(&ctl->abort, 1u);
      return true;
    }
  }
  if (spins > 32 && !((knobs >> 13) & 1)) __builtin_amdgcn_s_sleep(1);
  return false;
}

// Team formation + chain queue. Returns the team id (≥ 0) or -1 if this workgroup must exit. Called by all
// threads; thread 0 does the global traffic, the result is broadcast through LDS.
__device__ int join_team(TeamCtl* ctl, unsigned* err, int* sh, unsigned* sh_epoch, bool refuse = false) {
  if (threadIdx.x == 0) {
    *sh_epoch = ld_acq(&ctl->epoch);
    int res = -1;
    const unsigned x = xcc_id();
    if (x < kMaxTeams && !refuse) {
      const unsigned r = add_agent(&ctl->xcnt[x], 1u);
      if (r < (unsigned)kT) {
        res = (int)x * 64 + (int)r;        // team x, member r
        unsigned spins = 0;
        if (r == 0) {
          bool ok = false;
          while (true) {
            if (ld_acq(&ctl->xcnt[x]) >= (unsigned)kT) { ok = true; break; }
            if (++spins > (1u << 16)) break;
            __builtin_amdgcn_s_sleep(2);
          }
          st_rel(&ctl->state[x], ok ? 1u : 2u);
          if (!ok) res = -1;                 // no team on this XCD (placement/residency); others may drain the queue
        } else {
          unsigned s;
          while ((s = ld_acq(&ctl->state[x])) == 0) {
            if (++spins > (1u << 18)) break;
            __builtin_amdgcn_s_sleep(2);
          }
          if (s != 1) res = -1;
        }
      }
    }
    *sh = res;
  }
  __syncthreads();
  return *sh;
}

// Next chain for this team (all members agree). Returns chain id or -1 when the queue is drained / aborted.
__device__ int next_chain(TeamCtl* ctl, int team, int member, unsigned iter, int nch, int* sh) {
  if (threadIdx.x == 0) {
    int res = -1;
    unsigned spins = 0;
    if (member == 0) {
      // every member finished the previous chain (its exchange buffers are free again)
      while (ld_acq(&ctl->done[team]) < (unsigned)kT * iter) {
        if (ld_acq(&ctl->abort) || ++spins > (1u << 24)) { spins = ~0u; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      unsigned c = spins == ~0u ? 0xffffu : add_agent(&ctl->next_chain, 1u);
      if (c > 0xffffu) c = 0xffffu;
      st_rel(&ctl->chain[team], ((iter + 1) << 16) | c);
      res = (c < (unsigned)nch) ? (int)c : -1;
    } else {
      unsigned v;
      while (((v = ld_acq(&ctl->chain[team])) >> 16) != iter + 1) {
        if (ld_acq(&ctl->abort) || ++spins > (1u << 24)) { v = 0xffffu; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      const unsigned c = v & 0xffffu;
      res = (c < (unsigned)nch) ? (int)c : -1;
    }
    *sh = res;
  }
  __syncthreads();
  return *sh;
}

// Every workgroup calls this last (all threads). The last one to leave flags chains that no team processed
// (*err = 3), then resets the control block for the next launch on the same stream and advances the epoch.
__device__ void team_exit(TeamCtl* ctl, unsigned* err, int nch) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned e = add_agent(&ctl->exits, 1u);
    if (e == gridDim.x - 1) {
      if (ld_acq(&ctl->next_chain) < (unsigned)nch) st_rel(err, 3u);
      for (int i = 0; i < 16; ++i) st_rel(&ctl->xcnt[i], 0u);
      for (int i = 0; i < kMaxTeams; ++i) {
        st_rel(&ctl->state[i], 0u);
        st_rel(&ctl->chain[i], 0u);
        st_rel(&ctl->done[i], 0u);
      }
      st_rel(&ctl->next_chain, 0u);
      st_rel(&ctl->abort, 0u);
      st_rel(&ctl->exits, 0u);
      st_rel(&ctl->epoch, ld_acq(&ctl->epoch) + 1u);
    }
  }
}

// Queue depth. A hand-off tag is {epoch: 11 bits | (iter + 1) mod 32: 5 bits | step + 1: 16 bits}, iter counting the
// chains THIS team has pulled in the launch. A team that drains a queue of nch chains alone (no other team formed)
// runs iter = 0 … nch - 1, and the 5-bit field is different for any two of them exactly while nch ≤ 32: then no
// granule written anywhere in the launch can carry the tag another of its chains waits for, whatever the slots hold
// (rows a partial chain left unwritten, a chain cut short). At nch = 33, iter 0 and iter 32 share every tag. (With
// every chain writing all Bc rows and all S steps, a slot polled in iter i was last written in iter i - 1, whose
// field differs at any depth — but that argument leans on the chains being alike; the bound below leans on nothing.)
// The field value 0 (iter = 31) cannot match zero-initialised memory either: step + 1 ≥ 1. The exact plan refuses
// launches of more than kMaxQueue chains (plan_exact): 32 × 8 rows = 256 sequences per launch.
constexpr int kMaxQueue = 32;
__device__ __forceinline__ unsigned make_tagbase(unsigned epoch, unsigned iter) {
  return ((epoch & 0x7ffu) << 21) | (((iter + 1u) & 0x1fu) << 16);   // | (t + 1): 16 bits
}

// DCA_TEAM_KNOBS = pre_sleep | skip_outputs << 8 | probe_first << 9 | xp_step0 << 10 | no poll back-off sleep << 13
// (latency experiments only; bit 14 once selected a three-store forward output form and is no longer read);
// DCA_TEAM_FAIL=1 sets bit 11: no workgroup joins a team (fault injection: every chain left unprocessed → err 3);
// DCA_TEAM_PATIENT=1 sets bit 15: a 60 s instead of 2 s wall-clock hand-off timeout (spin_fail) for runs that share
// the GPU with another process's persistent kernels (bench.py DCA_SHARED_GPU rehearsals: two ranks' recurrences on
// one MI355X); a real lost hand-off still ends in the error, just later
inline int team_knobs() {
  const char* e = getenv("DCA_TEAM_KNOBS");
  const char* f = getenv("DCA_TEAM_FAIL");
  const char* p = getenv("DCA_TEAM_PATIENT");
  return (e ? atoi(e) : 0) | ((f && f[0] == '1') ? (1 << 11) : 0) | ((p && p[0] == '1') ? (1 << 15) : 0);
}

inline void plan(int B, int& nch, int& Bc, int& MT, int f32 = 0) {
  // Spread the sequences over all 8 teams (one chain per XCD) before packing rows into a chain: per-step latency
  // grows with rows per chain (more granules to gather and publish), measured B=8, H=512 fwd/bwd µs per step:
  // 1 chain × 8 rows 2.21/2.82, 2 × 4 2.09/2.57, 4 × 2 2.08/2.41, 8 × 1 2.08/2.26. Chains hold ≤ 32 rows; beyond
  // 8·32 sequences further chains queue behind the running ones.
  nch = B <= kMaxTeams * 32 ? (B < kMaxTeams ? B : kMaxTeams) : (B + 31) / 32;
  // F32 chains hold ≤ 16 rows (the backward's hi + lo gate-gradient images of 16 rows take 132 KB of LDS)
  if (f32 && (B + nch - 1) / nch > 16) nch = (B + 15) / 16;
  Bc = (B + nch - 1) / nch;
  MT = Bc <= 16 ? 1 : 2;
}

// The fp32-exact plan (`exact`): never leaves the exact VALU family, whatever B. As above up to 8 teams × kExactRows
// rows — one chain per XCD, rows per chain growing through 1, 2, 4, 8 (a chain of 3 or 5-7 rows runs the next form up
// with its last rows idle) — and value for value the plan above for B ≤ 32. Beyond that, ceil(B / kExactRows) chains
// of kExactRows rows which queue behind the 8 running ones (the last may be partial). `rows` (1, 2, 4, 8) forces the
// rows per chain (tests, scripts/exact_rows_bench.py); 0 lets the plan decide. False: not a launch this file runs.
constexpr int kExactRows = 8;           // rows of the largest exact VALU form
inline bool plan_exact(int B, int rows, int& nch, int& Bc, int& MT) {
  if (B < 1 || (rows != 0 && rows != 1 && rows != 2 && rows != 4 && rows != kExactRows)) return false;
  MT = 1;
  if (rows != 0) {
    Bc = rows;
    nch = (B + rows - 1) / rows;
  } else if (B <= kMaxTeams * kExactRows) {
    nch = B < kMaxTeams ? B : kMaxTeams;
    Bc = (B + nch - 1) / nch;
  } else {
    Bc = kExactRows;
    nch = (B + Bc - 1) / Bc;
  }
  return nch <= kMaxQueue;
}

// One front for every entry point: exact = 0 is plan() and takes no `rows`.
inline bool plan_any(int B, int f32, int exact, int rows, int& nch, int& Bc, int& MT) {
  if (exact) return f32 && plan_exact(B, rows, nch, Bc, MT);
  if (rows != 0) return false;
  plan(B, nch, Bc, MT, f32);
  return true;
}

// =============================================================================================================
// Kernel forms: which kernel runs for a launch, and why. A form is how the recurrent product is computed (Prod), how
// many rows of a chain one workgroup carries, H, and the activations (LIBM: libm expf / tanhf with IEEE division
// instead of v_exp_f32 + v_rcp_f32). The kernels are templates on exactly these four.
//   Bf16Mfma   bf16 W_hh, bf16 MFMA tiles of 16 rows (rows = 16 or 32), h exchanged in bf16
//   SplitMfma  fp32 W_hh split into hi + lo bf16, three MFMA products per tile (rows = 16), h exchanged in fp32
//   Valu4w     fp32 W_hh, exact fp32 VALU dot products on 4 waves, rows = 1, 2, 4 or 8
//   Valu8w     the same on 8 waves (two per SIMD), H = 512 only: the backward's form there. The forward has none: its
//              8-wave form measured slower every time (profiles/recurrence_bwd_handoff.md) and its 8-row one was 24 %
//              off float64 on its only run (profiles/exact_big_batch.md)
enum class Prod { Bf16Mfma, SplitMfma, Valu4w, Valu8w };
constexpr bool is_valu(Prod p) { return p == Prod::Valu4w || p == Prod::Valu8w; }
constexpr int form_threads(Prod p) { return p == Prod::Valu8w ? 512 : kThreads; }   // block size and launch bound

struct Form {
  Prod prod;
  int rows;                              // rows per chain the form carries; 0: no such kernel
  int h;
  bool libm;
};
constexpr bool operator==(const Form& a, const Form& b) {
  return a.prod == b.prod && a.rows == b.rows && a.h == b.h && a.libm == b.libm;
}
constexpr Form kNoForm = {Prod::Bf16Mfma, 0, 0, false};

// The form of a launch whose chains hold up to Bc rows (from the plan above). kNoForm: the launcher answers
// hipErrorInvalidValue, and launches nothing.
// * bf16 weights: MFMA tiles, one for ≤ 16 rows, else two.
// * fp32 weights and more than 4 rows (with `exact`: more than 8, which plan_exact never produces): split MFMA, one tile.
// * otherwise exact VALU: 1 / 2 / 4 / 8 rows for Bc = 1 / 2 / 3-4 / 5-8; eight waves for the backward at H = 512
//   (2069 vs 2137 µs per B=8, S=1400 call), else four.
// `precise` asks for the libm activations. Only the one-row VALU forms have them: with 2-8 rows per chain there is no
// such kernel and the launch is refused; the MFMA forms have no use for activations finer than their products and
// IGNORE the flag (a bf16 or a > 4-row launch with `precise` runs the same kernel as without).
constexpr Form select_form(bool f32, int Bc, int H, bool backward, bool precise, bool exact) {
  if (Bc < 1 || (H != 128 && H != 256 && H != 512)) return kNoForm;
  if (!f32) return Bc <= 32 ? Form{Prod::Bf16Mfma, Bc <= 16 ? 16 : 32, H, false} : kNoForm;
  if (Bc > (exact ? kExactRows : 4)) return Bc <= 16 ? Form{Prod::SplitMfma, 16, H, false} : kNoForm;
  const int rows = Bc == 1 ? 1 : (Bc == 2 ? 2 : (Bc <= 4 ? 4 : 8));
  if (precise && rows > 1) return kNoForm;
  return Form{(backward && H == 512) ? Prod::Valu8w : Prod::Valu4w, rows, H, precise};
}

// Every instantiated form, once: X(prod, rows, H, libm). The launchers compare select_form's answer against these
// lines and launch the one that matches; a form that is not listed does not exist.
#define DCA_TEAM_FWD_FORMS(X)                                                                           \
  X(Bf16Mfma, 16, 128, false)  X(Bf16Mfma, 16, 256, false)  X(Bf16Mfma, 16, 512, false)                 \
  X(Bf16Mfma, 32, 128, false)  X(Bf16Mfma, 32, 256, false)  X(Bf16Mfma, 32, 512, false)                 \
  X(SplitMfma, 16, 128, false) X(SplitMfma, 16, 256, false) X(SplitMfma, 16, 512, false)                \
  X(Valu4w, 1, 128, false)     X(Valu4w, 1, 256, false)     X(Valu4w, 1, 512, false)                    \
  X(Valu4w, 1, 128, true)      X(Valu4w, 1, 256, true)      X(Valu4w, 1, 512, true)                     \
  X(Valu4w, 2, 128, false)     X(Valu4w, 2, 256, false)     X(Valu4w, 2, 512, false)                    \
  X(Valu4w, 4, 128, false)     X(Valu4w, 4, 256, false)     X(Valu4w, 4, 512, false)                    \
  X(Valu4w, 8, 128, false)     X(Valu4w, 8, 256, false)     X(Valu4w, 8, 512, false)
#define DCA_TEAM_BWD_FORMS(X)                                                                           \
  X(Bf16Mfma, 16, 128, false)  X(Bf16Mfma, 16, 256, false)  X(Bf16Mfma, 16, 512, false)                 \
  X(Bf16Mfma, 32, 128, false)  X(Bf16Mfma, 32, 256, false)  X(Bf16Mfma, 32, 512, false)                 \
  X(SplitMfma, 16, 128, false) X(SplitMfma, 16, 256, false) X(SplitMfma, 16, 512, false)                \
  X(Valu4w, 1, 128, false)     X(Valu4w, 1, 256, false)     X(Valu8w, 1, 512, false)                    \
  X(Valu4w, 1, 128, true)      X(Valu4w, 1, 256, true)      X(Valu8w, 1, 512, true)                     \
  X(Valu4w, 2, 128, false)     X(Valu4w, 2, 256, false)     X(Valu8w, 2, 512, false)                    \
  X(Valu4w, 4, 128, false)     X(Valu4w, 4, 256, false)     X(Valu8w, 4, 512, false)                    \
  X(Valu4w, 8, 128, false)     X(Valu4w, 8, 256, false)     X(Valu8w, 8, 512, false)
constexpr bool form_listed(Form f, bool backward) {
#define DCA_X(P, ROWS, H_, LIBM) || f == Form{Prod::P, ROWS, H_, LIBM}
  return backward ? (false DCA_TEAM_BWD_FORMS(DCA_X)) : (false DCA_TEAM_FWD_FORMS(DCA_X));
#undef DCA_X
}

// select_form's outcomes, pinned (f32, Bc, H, backward, precise, exact), and each of them instantiated
#define DCA_PIN(BWD, WANT, ...) \
  static_assert(select_form(__VA_ARGS__) == (WANT) && form_listed(select_form(__VA_ARGS__), BWD) == ((WANT).rows != 0))
DCA_PIN(false, (Form{Prod::Bf16Mfma, 16, 512, false}), false, 16, 512, false, false, false);
DCA_PIN(true, (Form{Prod::Bf16Mfma, 32, 128, false}), false, 17, 128, true, false, false);
DCA_PIN(false, (Form{Prod::Bf16Mfma, 16, 256, false}), false, 1, 256, false, true, false);      // precise: ignored
DCA_PIN(false, (Form{Prod::SplitMfma, 16, 512, false}), true, 5, 512, false, false, false);
DCA_PIN(true, (Form{Prod::SplitMfma, 16, 512, false}), true, 16, 512, true, true, false);       // precise: ignored
DCA_PIN(true, (Form{Prod::SplitMfma, 16, 256, false}), true, 9, 256, true, false, true);        // (not a plan_exact chain)
DCA_PIN(false, (Form{Prod::Valu4w, 1, 512, false}), true, 1, 512, false, false, false);         // forward: four waves
DCA_PIN(true, (Form{Prod::Valu8w, 1, 512, false}), true, 1, 512, true, false, false);           // backward at 512: eight
DCA_PIN(true, (Form{Prod::Valu4w, 1, 256, false}), true, 1, 256, true, false, false);
DCA_PIN(false, (Form{Prod::Valu4w, 2, 128, false}), true, 2, 128, false, false, false);
DCA_PIN(true, (Form{Prod::Valu8w, 4, 512, false}), true, 3, 512, true, false, false);
DCA_PIN(false, (Form{Prod::Valu4w, 4, 256, false}), true, 4, 256, false, false, true);
DCA_PIN(false, (Form{Prod::Valu4w, 8, 512, false}), true, 5, 512, false, false, true);          // exact: 5-8 rows stay VALU
DCA_PIN(true, (Form{Prod::Valu8w, 8, 512, false}), true, 8, 512, true, false, true);
DCA_PIN(false, (Form{Prod::Valu4w, 1, 128, true}), true, 1, 128, false, true, false);           // LIBM = precise
DCA_PIN(true, (Form{Prod::Valu8w, 1, 512, true}), true, 1, 512, true, true, true);
DCA_PIN(false, kNoForm, true, 2, 512, false, true, false);                                      // precise, 2-8 rows: refused
DCA_PIN(true, kNoForm, true, 8, 512, true, true, true);
DCA_PIN(false, kNoForm, true, 17, 512, false, false, false);                                    // (not a plan chain)
DCA_PIN(false, kNoForm, false, 8, 384, false, false, false);
#undef DCA_PIN

}  // namespace

// Exchange-buffer bytes of a launch (defined beside the forward launcher; the backward launcher checks against it)
extern "C" size_t dca_lstm_team_workspace(int B, int H, int backward, int f32, int exact, int rows);
