// picp_persistent.hip -- the whole exec/icp_test.cpp:88-107 loop in ONE launch, for batches whose
// blocks all fit on the chip at once (a single 100k-1M frame, a few frames).
//
// Why: with one launch per round the critical path of a round is launch gap + a chip-wide
// re-read of every block partial + the serial solve (tools/stamps.py).  Here each
// block loads its slice of the frame into REGISTERS once (never re-read from HBM), and each
// round costs one fan-in and one fan-out inside the launch:
//   1. every block linearizes its slice at the current pose and publishes its 32-float partial
//      as 32 granules {tag = round+1, value} (8-byte relaxed agent-scope atomic stores: the R2
//      hand-off of cdna_hip_programming.md Guideline 16 -- the data IS the flag, no fences);
//   2. the problem's solver blocks (its first PICP_PSOLVERS blocks, one per XCD under round-robin
//      placement) each sweep those granules until every tag matches, sum them in a FIXED order
//      (deterministic: every solver gets the same bits), solve the damped 6x6 system and apply
//      the update (picp_solve6.h: finish_round), then publish the new pose as 16 granules
//      {round+1, word} twice: kept in their XCD's L2 and agent-scope;
//   3. every other block polls its solver's 16 pose granules (one wave: a ring of polls in
//      flight, PICP_POSE_POLLS of them with one item per lane and two otherwise) -- the L2 copy
//      once the first round has shown that it runs on the solver's XCD -- then starts the next round.
// Correctness does not depend on placement or timing: only tags are trusted.  Blocks must be
// co-resident (the host caps the grid at the CU count with ~110 VGPRs / 10 KB LDS per block),
// every spin is bounded by a per-round s_memrealtime deadline (timeout -> error word, loop exits), and
// tags are offset by a per-problem round counter kept on the device (tagbase), so granules left
// by earlier launches never match and no memset runs between launches.
#include "picp_item.h"
#include "picp_launch.h"
#include "picp_pose.h"
#include "picp_solve6.h"
#include "picp_variant.h"
#include "picp_wave.h"

using namespace picp;

typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) unsigned int gu32_t;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PICP_MAX_PBLK 256   // max blocks per problem in this mode (sweep registers)
#define PICP_PBLOCK 512     // the partition's unit: npt items per lane of a 512-thread block
// (npt 8 as 1024 threads x 4 items did not move C3: DESIGN.md Appendix A, "1024 x 4".)
// Followers' pose wait, two and more items per lane: two polls in flight this many s_sleep units
// (64 clocks) apart
#define PICP_POSE_STAGGER 8
// Followers' pose wait, one item per lane: a ring of PICP_POSE_POLLS polls in flight, first issued
// PICP_POSE_SPACING s_sleep units apart: one PICP_POSE_POLLS-th of the round trip of an sc1 load
// served by the L2, which measures 80-120 ns (profiles/r16/pose_polls/pst_parent_c2.log).  Each is
// re-issued as it is checked, so the spacing holds.  Two polls is the measured best: every poll
// more in flight costs the round about 50 ns (the 24 followers of an XCD poll one L2 line, and the
// solver's store and the poll that meets it queue behind them), one fewer 30 ns, and no spacing
// from 2 to 8 units tells.  Both can be set from the make
// line for A/B builds; 0 polls compiles the two-poll wait of the other kernels.
#ifndef PICP_POSE_POLLS
#define PICP_POSE_POLLS 2
#endif
#ifndef PICP_POSE_SPACING
#define PICP_POSE_SPACING 2
#endif
static_assert(PICP_POSE_POLLS >= 0 && PICP_POSE_POLLS <= 16, "PICP_POSE_POLLS: 1 to 16 polls in flight, 0: the two-poll wait");
// (The ring's first poll issued a lag after the block's post-linearize barrier, as the sweep's
// first pass is: every lag from 200 ns on lost 1 %, DESIGN.md Appendix A "pose lag".)
// The solvers' sweep with two passes in flight, PICP_SWEEP_STAGGER x 64 clocks apart.
// Each pass loads every pending granule pair (the others point past the buffer's
// range: no memory access, a zero), so both passes' loads are unconditional and the waits count
// exactly one pass.  C3 150.5k -> 156.5k it/s (8 x 64 clocks; 16: 155k); with one item per lane
// (C2) -2 %, so it starts at PICP_SWEEP_MIN_NPT items (profiles/r05/sweep_stagger/).
// As compiled, take(gb) is scheduled above issue(ga), so after the first iteration the two
// passes are issued back to back and both are waited for; with the order forced (a scheduling
// barrier after issue(ga)) C3 lost 4.5 %, with one pass only 2.4 % (DESIGN.md Appendix A, round
// 11), so the source and that schedule stay.
#define PICP_SWEEP_STAGGER 8
#define PICP_SWEEP_MIN_NPT 2  // the staggered sweep from this many items per lane on
// The first sweep pass of every solver wave is issued this long after the block's post-linearize
// barrier (the kernel's sweep_lag; PICP_SWEEP_LAG_NS overrides it) where the sweep is not staggered
// and the problem has follower blocks.  The followers start a round one pose hand-off after their
// solver, so the last of them publishes about 0.6 us after the solver's barrier; the measured
// curve on the 100k frame (profiles/r13/round/ab_lag_curve.log) has its best at 600 ns, within
// 1 % of it from 550 to 650 and above no lag from 450 to 700.  With two staggered passes in flight
// (PICP_SWEEP_MIN_NPT items per lane and more) no lag from 0 to 600 ns moved C3 and longer ones
// lost, and the lag's code in those kernels cost C3 2 %, so they are compiled without it.
#define PICP_SWEEP_LAG_NS_DEFAULT 600
#define PICP_POSE_GRAN 16   // pose granules per set: R(9) t(3) done(1) solver XCC id(1) pad(2)
// Solver blocks per problem.  Blocks kb and kb + 8j share an XCD under round-robin placement, so solver
// kb & 7 publishes where its followers' polls are L2 hits instead of fabric round trips: an
// agent-scope (sc1) store drops its line from the writer's L2 (MI355X_MICROARCH.md), a
// workgroup-scope (sc0) store keeps it there.  Placement is not guaranteed, so the solver also
// publishes agent-scope and carries its XCC id; a follower on another XCD polls that copy.
#define PICP_PSOLVERS 8
// each solver owns two pose sets (its L2 copy and its agent-scope copy) of the problem's region
static_assert(2 * PICP_PSOLVERS <= PICP_POSE_SETS, "PICP_PSOLVERS needs 2 pose sets each (picp_internal.h)");
// (A timeout in one solver ends its followers' waits; the other solvers then wait out their own
// deadline before the error word forces the re-run.  Checking the error word every 32 passes of an
// incomplete sweep would end them sooner, but that check in the spin loops measured C2 -2.6 %,
// C3 -1.2 % on the normal path (profiles/r06/t4/ab.log), so timeouts keep the two-window cost.)
// raw buffer load aux: sc1 (bit 4: bypass L1, served by L2 / the fabric) | volatile (bit 31:
// never hoisted out of a spin loop)
#define PICP_AUX_SC1_VOLATILE ((int)(16u | 0x80000000u))
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Diagnostic build only (-DPICP_STAMPS): s_memrealtime per phase of rounds (epochs) 11 and 12.
#ifdef PICP_STAMPS
// slots 0-7 as below; 8: a solver's pose stores issued (wave 0); a follower: 9, 10 one pose poll of
// its own, issued and returned (the round trip of an sc1 load, taken right after the publish when
// no pose can be there yet), 11: whether it polls the L2 copy (s_l2)
#define PICP_PSTAMP_SLOTS 12
__device__ unsigned long long picp_pstamps[2][256][PICP_PSTAMP_SLOTS];
#define PSTAMP_T(k, t)                                                                         \
  do {                                                                                         \
    if (threadIdx.x == (t) && (epoch == 11 || epoch == 12) && blockIdx.x < 256)                \
      picp_pstamps[epoch - 11][blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();               \
  } while (0)
#define PSTAMP(k) PSTAMP_T(k, 0)
#define PSTAMP_VAL(k, val)                                                                     \
  do {                                                                                         \
    if (threadIdx.x == 0 && (epoch == 11 || epoch == 12) && blockIdx.x < 256)                  \
      picp_pstamps[epoch - 11][blockIdx.x][k] = (val);                                         \
  } while (0)
// What a round waits for besides its hand-offs (slots 6 and 7).  A follower: thread 64 (wave 1,
// which never polls) stamps the round start (6) and the pose barrier (7) beside wave 0's stamps
// 0 and 2, so the stretch barrier -> next round start can be compared between the polling wave
// and one that has nothing in flight.  A solver: thread 0 at the sweep's exit (6) and after the
// double sums (7), the stretch that holds the wait for a sweep pass still in flight.
#define PSTAMP_W1(k) PSTAMP_T(k, 64)
extern "C" hipError_t picp_debug_pstamps(unsigned long long* out, size_t n_words);
// the leader's sweep, per wave (its first lane still in the sweep, so the passes are the wave's and
// not one lane's): each pass's issue (slot 2k) and return (2k + 1) times, the post-linearize
// barrier (62) and the pass count (63), rounds 11 and 12
#define PICP_SWS_BAR 62
#define PICP_SWS_COUNT 63
__device__ unsigned long long picp_sweepstamps[2][PICP_PBLOCK / 64][64];
#define SWSTAMP_V(k, val)                                                                      \
  do {                                                                                         \
    const int k_ = (k); /* once: the sweep passes a counter's post-increment */                \
    if (blockIdx.x == 0 && (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1 &&   \
        (epoch == 11 || epoch == 12) && k_ < 64)                                               \
      picp_sweepstamps[epoch - 11][threadIdx.x >> 6][k_] = (val);                               \
  } while (0)
#define SWSTAMP(k)                                                                             \
  do {                                                                                         \
    const int kp_ = (k);                                                                       \
    if (kp_ < PICP_SWS_BAR) SWSTAMP_V(kp_, __builtin_amdgcn_s_memrealtime());                   \
  } while (0)
#define SWSTAMP_BAR() SWSTAMP_V(PICP_SWS_BAR, __builtin_amdgcn_s_memrealtime())
#define SWSTAMP_COUNT(n) SWSTAMP_V(PICP_SWS_COUNT, (unsigned long long)(n))
extern "C" hipError_t picp_debug_sweepstamps(unsigned long long* out, size_t n_words);
#else
#define SWSTAMP(k) \
  do {             \
  } while (0)
#define SWSTAMP_BAR() \
  do {                \
  } while (0)
#define SWSTAMP_COUNT(n) \
  do {                   \
  } while (0)
#define PSTAMP(k) \
  do {            \
  } while (0)
#define PSTAMP_W1(k) \
  do {               \
  } while (0)
#endif

__device__ __forceinline__ unsigned long long granule(unsigned epoch, float v) {
  return ((unsigned long long)epoch << 32) | (unsigned long long)__float_as_uint(v);
}

// Word (lane & 15) of 16 words that every lane holds: four levels of bit selects on the lane id
// (a v_bfe_i32 mask and 8, 4, 2, 1 v_bfi_b32).  No lane mask in an SGPR pair: the fourteen
// (lane == i) selects this replaces kept theirs across the round loop, spilled, and reloaded each
// (two v_readlane_b32 and an s_nop) in front of the pose stores.  The masks come from inline
// assembly so that they are made where they are used (as plain C they are hoisted out of the
// round loop into four VGPRs) and the selects are not turned back into compares.
__device__ __forceinline__ unsigned lane_word16(const unsigned (&w)[16], int lane) {
  unsigned v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = w[k];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    unsigned m;  // bit b of the lane in every bit
    asm volatile("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(lane), "n"(b));
#pragma unroll
    for (int k = 0; k < (8 >> b); ++k) v[k] = (v[2 * k + 1] & m) | (v[2 * k] & ~m);
  }
  return v[0];
}

// (hand-off polls run back to back: a pause between them lost, DESIGN.md Appendix A "poll sleep")
__device__ __forceinline__ bool timed_out(unsigned long long deadline) {
  return __builtin_amdgcn_s_memrealtime() > deadline;
}

template <int NPT, int PH, int BS>
__global__ __launch_bounds__(BS) void picp_persistent_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
    const float* __restrict__ U, const float* __restrict__ V, const PicpArgs A,
    const PicpState* __restrict__ st_in, PicpState* __restrict__ st_out,
    unsigned long long* gpart, unsigned long long* gpose, unsigned int* err, unsigned int* tagbase,
    unsigned long long sweep_lag, unsigned long long timeout_ticks) {
  // sweep_lag (s_memrealtime ticks, 10 ns): the solvers' first sweep pass is issued this long after
  // the block's post-linearize barrier (below).  It has the kernel-argument slot of the deleted
  // arrival counter, so timeout_ticks keeps its kernarg offset (moving it reordered the NPT = 8
  // schedule, profiles/r07/prune/ab.log).
  __shared__ double s_red[PICP_NPART][BS / 64];  // term-major: one row per combining lane
  __shared__ float s_tot[PICP_NPART];
  __shared__ float s_wave[BS / 64][PICP_NPART];
  // The round's control words, one 16-word row so that a follower's polling wave stores what it
  // received with one LDS store per lane (lane l < 14 writes word l): the pose, the done flag and
  // whether this follower runs on its solver's XCD (then it polls the L2 copy of the pose).
  // (As three objects the stores were six exec-mask branches in front of the pose barrier.)
  __shared__ unsigned s_ctl[16];
  float* const s_pose = (float*)s_ctl;  // words 0-11: R (9), t (3)
  int& s_done = *(int*)&s_ctl[12];
  int& s_l2 = *(int*)&s_ctl[13];
  __shared__ int s_tmo;  // a wait of this block timed out (the error word is for the host)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nblk = A.nblk_u;
  const int p = (int)blockIdx.x / nblk;
  const int kb = (int)blockIdx.x - p * nblk;
  const int first = kb * A.ipb;
  const int count = max(0, min(A.ipb, A.n_u - first));
  const int64_t base = (int64_t)p * A.stride_u + first;
  const bool leader = (kb == 0);                 // keeps the loop state and the tag base
  const bool solver = (kb < PICP_PSOLVERS);      // sweeps, solves and publishes the pose
  const int sg = kb % PICP_PSOLVERS;             // this block's solver
  // partial granules are double-buffered by round parity, so correctness does not rest on the
  // leader having swept round r before any block publishes round r+1
  const size_t part_stride = (size_t)gridDim.x * PICP_NPART;
  gu64_t* my_part0 = ((gu64_t*)gpart) + (size_t)blockIdx.x * PICP_NPART;
  gu64_t* prob_part0 = ((gu64_t*)gpart) + (size_t)p * nblk * PICP_NPART;
  gu64_t* prob_pose = ((gu64_t*)gpose) + (size_t)p * PICP_POSE_SETS * PICP_POSE_GRAN;
  gu64_t* pose_l2 = prob_pose + (size_t)(2 * sg) * PICP_POSE_GRAN;      // kept in the XCD's L2
  gu64_t* pose_gl = prob_pose + (size_t)(2 * sg + 1) * PICP_POSE_GRAN;  // agent scope
  unsigned my_xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
  gu32_t* errw = ((gu32_t*)err);
  // Granule tags are tbase + round.  tbase is the problem's count of rounds run by every earlier
  // launch on these buffers (its leader advances it after the last round), so tags never repeat
  // and no memset node has to clear the granules before each launch.
  gu32_t* tbase_p = ((gu32_t*)tagbase) + p;
  const unsigned tbase = __hip_atomic_load(tbase_p, RLX_AGENT);
  // (A per-problem arrival counter the solvers waited on before the sweep halved C2 and C3:
  // DESIGN.md Appendix A, "arrival counter".)

  // this block's slice, loaded once into registers (coalesced: item = tid + k*BLOCK)
  float xs[NPT], ys[NPT], zs[NPT], us[NPT], vs[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * BS;
    const int ic = min(i, max(count - 1, 0));
    xs[k] = X[base + ic];
    ys[k] = Y[base + ic];
    zs[k] = Z[base + ic];
    us[k] = U[base + ic];
    vs[k] = V[base + ic];
  }

  if (tid == 0) {  // initial state, as launch 0 of the multi-launch path
    PicpState s = st_in[p];
    s.chi_prev = FLT_MAX;  // exec/icp_test.cpp:89
    s.chi_in = s.chi_out = 0.0f;
    s.n_in = s.n_proj = 0;
    s.rounds = 0;
    s.done = (A.max_rounds <= 0) ? 1 : 0;
    s.ok = 1;
    s.converged = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s_pose[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s_pose[9 + i] = s.t[i];
    s_done = s.done;
    s_tmo = 0;
    s_l2 = 0;
    if (leader && s.done) st_out[p] = s;
  }
  __syncthreads();

  Cam C;
  cam_load(A.K, A.maxx, A.maxy, C);
  const float thr = A.threshold;
  const float inv_thr = 1.0f / thr;
  const bool keep = A.keep_outliers != 0;
  const TotalLane tl = total_lane(A, lane);  // the finishing wave: lane e converts total e
  // The finish by lanes (below) with one item per lane, where the linearize leaves registers to
  // spare: its per-lane constants and the word of pose granule 13 (this solver's XCC id) are made
  // once and stay in VGPRs.  With more items per lane the kernels keep the uniform finish: their
  // registers are bound (the constants live through the linearize spilled; read from LDS each
  // round the finish by lanes measured C3 inside the uniform one's band, profiles/r13/round/
  // ab_leave_one_out.log), and as compiled they are instruction for instruction what they were.
  constexpr bool LANES = (NPT == 1);
  FinishLanes fl = {};
  unsigned xcc_word = 0u;
  if constexpr (LANES) {
    fl = finish_lanes(lane);
    xcc_word = lane == 13 ? my_xcc : 0u;
    asm volatile("" : "+v"(xcc_word));
  }

  // The slice has landed before the first round: the round loop's waits then count nothing that
  // was issued before it, so a follower's poll left in flight (below) is never waited for by the
  // linearize's first use of an item.
#pragma unroll
  for (int k = 0; k < NPT; ++k) asm volatile("" ::"v"(xs[k]), "v"(ys[k]), "v"(zs[k]), "v"(us[k]), "v"(vs[k]));

  float chi_prev = FLT_MAX;  // the leader's loop state besides the pose (exec/icp_test.cpp:89)
  unsigned long long pose_sink = 0, pa = 0, pb = 0;  // the follower's pose polls
  // ... with one item per lane: the ring (pa and pb stay unused there)
  constexpr bool RINGED = LANES && PICP_POSE_POLLS > 0;
  constexpr int RING = RINGED ? PICP_POSE_POLLS : 1;
  unsigned long long ring[RING] = {};
  for (unsigned epoch = 1; !s_done; ++epoch) {
    // every wait of this round is bounded from the round's start (a whole solve may take far
    // longer than timeout_ticks at large max_rounds; one round never does)
    const unsigned long long deadline = __builtin_amdgcn_s_memrealtime() + timeout_ticks;
    // ---- 1. linearize the slice at the current pose, publish the block partial ----
    PSTAMP(0);
    if (!solver) PSTAMP_W1(6);
    Pose T;
    pose_load(s_pose, s_pose + 9, T);
    float v[PICP_NPART];
    Cnt nc = {0u, 0u};  // the wave's n_in / n_proj (scalar unit)
    if constexpr (NPT == 1) {  // one item per lane: the scalar path (latency-bound C2 frames)
      Acc a;
#pragma unroll
      for (int i = 0; i < 21; ++i) a.h[i] = 0.0f;
#pragma unroll
      for (int i = 0; i < 6; ++i) a.b[i] = 0.0f;
      a.chi_in = a.chi_out = 0.0f;
      accumulate<PH>(T, C, thr, inv_thr, keep, xs[0], ys[0], zs[0], us[0], vs[0], tid < count, a, nc);
#pragma unroll
      for (int i = 0; i < 21; ++i) v[PICP_P_H + i] = a.h[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) v[PICP_P_B + i] = a.b[i];
      v[PICP_P_CHI_IN] = a.chi_in;
      v[PICP_P_CHI_OUT] = a.chi_out;
      v[PICP_P_N_IN] = 0.0f;
      v[PICP_P_N_PROJ] = 0.0f;
      v[31] = 0.0f;
    } else {  // NPT register-resident items per lane
      if constexpr (acc_pairs(NPT)) {
        Acc2 a;
        acc2_zero(a);
        accumulate_regs<PH, NPT>(T, C, thr, inv_thr, keep, xs, ys, zs, us, vs, tid, BS, count, a, nc);
        acc2_fold(a, v);
      } else {
        Acc a;
        acc_zero(a);
        accumulate_regs1<PH, NPT>(T, C, thr, inv_thr, keep, xs, ys, zs, us, vs, tid, BS, count, a, nc);
        acc_fold(a, v);
      }
    }
    const float wsum = wave_counts(wave_reduce32(v, lane), lane, nc);
    if ((lane & 1) == 0) s_wave[wave][lane >> 1] = wsum;
    __syncthreads();
    // A solver's first sweep pass is a round trip of 0.6-1.1 us, and whatever it misses costs a
    // second one.  Issued straight after this barrier (waves 1-7 have no publish to do) it leaves
    // before the later followers have published, so every solver wave issues it at one time
    // point instead, sweep_lag after the barrier: wave 0 waits only what is left after its
    // publish.  Only tags are trusted, so the lag is never a matter of correctness: a lag too short
    // costs the second pass it was meant to save, one too long its own length.
    constexpr bool TIMED = (NPT < PICP_SWEEP_MIN_NPT);
    unsigned long long sweep_at = 0;
    if constexpr (TIMED) {
      if (solver && sweep_lag) sweep_at = __builtin_amdgcn_s_memrealtime() + sweep_lag;
    }
    if (solver) SWSTAMP_BAR();
    if (tid < PICP_NPART) {
      float sum = s_wave[0][tid];
#pragma unroll
      for (int w = 1; w < BS / 64; ++w) sum += s_wave[w][tid];
      __hip_atomic_store(my_part0 + (epoch & 1) * part_stride + tid, granule(tbase + epoch, sum), RLX_AGENT);
    }
    PSTAMP(1);

    if (solver) {
      // ---- 2. sweep the problem's partials: 16-B sc1 loads of granule pairs (2c, 2c+1) of
      //         blocks g + NG*i (c = tid&15, g = tid>>4); each 8-B half carries its own tag ----
      const int c = tid & 15, g = tid >> 4;
      constexpr int NG = BS / 16;  // block groups swept in parallel
      constexpr int MAXG = PICP_MAX_PBLK / NG;
      const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(prob_part0 + (epoch & 1) * part_stride), 0, nblk * PICP_NPART * 8, 0x00020000);
      u32x4 gv[MAXG];
      // re-poll only the pairs whose tags have not both matched yet: a full 50 KB sweep costs
      // ~0.5 us at one block's share of the fabric, a re-poll of the few late blocks far less
      // (a probe-first sweep -- only each block's last pair polled until it arrives -- measured
      // 17 % slower on C2: the pass is a round trip, not bandwidth, and the probe adds one)
      unsigned pending = 0;
#pragma unroll
      for (int i = 0; i < MAXG; ++i) {
        gv[i] = (u32x4){0u, 0u, 0u, 0u};
        if (g + NG * i < nblk) pending |= 1u << i;
      }
      [[maybe_unused]] int npass = 0;  // sweep passes (diagnostic stamps)
      if constexpr (TIMED) {
        if (sweep_lag) {  // never past the round's deadline
          const unsigned long long until = sweep_at < deadline ? sweep_at : deadline;
          while (__builtin_amdgcn_s_memrealtime() < until) __builtin_amdgcn_s_sleep(1);
        }
      }
      constexpr int SWEEP_ST = (NPT >= PICP_SWEEP_MIN_NPT) ? PICP_SWEEP_STAGGER : 0;
      if constexpr (SWEEP_ST > 0) {
        u32x4 ga[MAXG], gb[MAXG];
        auto issue = [&](u32x4* gg, unsigned want) {
#pragma unroll
          for (int i = 0; i < MAXG; ++i)
            gg[i] = __builtin_amdgcn_raw_buffer_load_b128(
                rsrc, (want & (1u << i)) ? ((g + NG * i) * PICP_NPART + 2 * c) * 8 : 0x7ffffff0, 0,
                PICP_AUX_SC1_VOLATILE);
        };
        auto take = [&](const u32x4* gg, unsigned want) {
#pragma unroll
          for (int i = 0; i < MAXG; ++i)
            if ((want & pending & (1u << i)) && gg[i][1] == tbase + epoch && gg[i][3] == tbase + epoch) {
              gv[i] = gg[i];
              pending &= ~(1u << i);
            }
        };
        [[maybe_unused]] int nissue = 0;  // passes issued / taken (diagnostic stamps)
        unsigned wa = pending, wb;
        SWSTAMP(2 * nissue++);
        issue(ga, wa);
        __builtin_amdgcn_s_sleep(SWEEP_ST);
        wb = pending;
        SWSTAMP(2 * nissue++);
        issue(gb, wb);
        for (;;) {
          take(ga, wa);
          SWSTAMP(2 * npass++ + 1);
          if (!pending) break;
          wa = pending;
          SWSTAMP(2 * nissue++);
          issue(ga, wa);
          take(gb, wb);
          SWSTAMP(2 * npass++ + 1);
          if (!pending) break;
          wb = pending;
          SWSTAMP(2 * nissue++);
          issue(gb, wb);
          if (timed_out(deadline)) {
            __hip_atomic_store(errw, 1u, RLX_AGENT);
            s_tmo = 1;
            break;
          }
        }
      } else {
        for (;;) {
          const unsigned want = pending;  // issue every pending load before checking any tag
          SWSTAMP(2 * npass);
#pragma unroll
          for (int i = 0; i < MAXG; ++i)
            if (want & (1u << i))
              gv[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ((g + NG * i) * PICP_NPART + 2 * c) * 8, 0,
                                                             PICP_AUX_SC1_VOLATILE);
#pragma unroll
          for (int i = 0; i < MAXG; ++i)
            if ((want & (1u << i)) && gv[i][1] == tbase + epoch && gv[i][3] == tbase + epoch) pending &= ~(1u << i);
          SWSTAMP(2 * npass + 1);
          ++npass;
          if (!pending) break;
          if (timed_out(deadline)) {
            __hip_atomic_store(errw, 1u, RLX_AGENT);
            s_tmo = 1;
            break;
          }
        }
      }
      SWSTAMP_COUNT(npass);
      // every gv[i]: a block's granule pair, or the zeros it started with where g + NG*i is past
      // the problem's blocks (never loaded).  Adding those zeros is exact and the sum cannot be
      // -0 (it starts at +0), so no guard per i: the same bits, i ascending
      PSTAMP(6);
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
      for (int i = 0; i < MAXG; ++i) {
        acc0 += (double)__uint_as_float(gv[i][0]);
        acc1 += (double)__uint_as_float(gv[i][2]);
      }
      // the wave's four groups (lanes c, 16+c, 32+c, 48+c) first: every lane ends with the same
      // (a0+a1)+(a2+a3) (IEEE addition commutes), so the order stays fixed
      PSTAMP(7);
      acc0 = wave_add_xor_f64<16>(acc0);
      acc1 = wave_add_xor_f64<16>(acc1);
      acc0 = wave_add_xor_f64<32>(acc0);
      acc1 = wave_add_xor_f64<32>(acc1);
      if (lane < 16) {
        s_red[2 * c][wave] = acc0;
        s_red[2 * c + 1][wave] = acc1;
      }
      __syncthreads();
      PSTAMP(2);
      // ---- finish the round in wave 0 only: lanes < 32 combine the groups (fixed order), then
      //      the wave finishes the round (every lane computes the same values) and
      //      lanes 0-15 each publish their pose word directly; the other waves meet wave 0 at
      //      the barrier below, off the publish path ----
      if (wave == 0) {
        if constexpr (LANES) {
          if (lane < PICP_NPART) {
            double ws[BS / 64];  // every load issued before the first add
#pragma unroll
            for (int w = 0; w < BS / 64; ++w) ws[w] = s_red[lane][w];
            double t = ws[0];
#pragma unroll
            for (int w = 1; w < BS / 64; ++w) t += ws[w];
            s_tot[lane] = total_word(tl, t);  // lane e converts total e
          }
          __builtin_amdgcn_wave_barrier();
          {
            // the wave finishes the round: the solve and the rotation in every lane, then lane
            // l < 12 computes word l of the new pose from its three words of s_pose (read per lane
            // ahead of the solve; s_pose changes only below); chi_prev stays in registers
            RoundOut o;
            PSTAMP(4);
            const float w = finish_round_lanes(A, s_tot, s_pose, (int)epoch, fl, chi_prev, o);
            PSTAMP(5);
            // (read here, after the solve: hoisted to the combine's loads it measured no faster,
            // DESIGN.md Appendix A "s_tmo read early")
            if (s_tmo) o.done = 1;  // a sweep timed out
            // ---- publish the new pose (and the done flag): lane l < 16 owns word l -- the pose
            //      (0-11), done (12), this solver's XCC id (13), zero (14, 15) ----
            const unsigned cw = (__float_as_uint(w) & (fl.row[0] | fl.row[1] | fl.row[2])) |
                                ((unsigned)o.done & fl.m12) | xcc_word;
            if (lane < PICP_POSE_GRAN) {
              const unsigned long long gw = ((unsigned long long)(tbase + epoch) << 32) | cw;
              __hip_atomic_store(pose_l2 + lane, gw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_store(pose_gl + lane, gw, RLX_AGENT);
            }
            PSTAMP(8);
            if (lane < 13) s_ctl[lane] = cw;  // the pose and s_done (word 13, s_l2, is the follower's)
            if (o.done && leader) {
              if (lane < 12) ((unsigned*)(st_out + p))[lane] = cw;  // R (9), t (3): lane l owns word l
              if (lane == 0) {
                store_state_rest(st_out + p, chi_prev, o, (int)epoch);
                // every block of the problem read tbase before publishing round 1, and this is
                // after its last round: the next launch's tags start past this one's
                __hip_atomic_store(tbase_p, tbase + epoch, RLX_AGENT);
              }
            }
          }
        } else {
          // the pose: kept from the round start when the linearize leaves registers to spare (one
          // item per lane), else re-read here (three 16-B LDS loads, landing during the combine):
          // kept live through a register-bound linearize it spilled; s_pose changes only after the
          // finish
          float pr[9], pt[3];
          if constexpr (NPT == 1) {
            pr[0] = T.r00; pr[1] = T.r10; pr[2] = T.r20; pr[3] = T.r01; pr[4] = T.r11; pr[5] = T.r21;
            pr[6] = T.r02; pr[7] = T.r12; pr[8] = T.r22; pt[0] = T.t0; pt[1] = T.t1; pt[2] = T.t2;
          } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) pr[i] = s_pose[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) pt[i] = s_pose[9 + i];
          }
          if (lane < PICP_NPART) {
            double ws[BS / 64];  // every load issued before the first add
#pragma unroll
            for (int w = 0; w < BS / 64; ++w) ws[w] = s_red[lane][w];
            double t = ws[0];
#pragma unroll
            for (int w = 1; w < BS / 64; ++w) t += ws[w];
            s_tot[lane] = total_word(tl, t);  // lane e converts total e
          }
          __builtin_amdgcn_wave_barrier();
          {
            // the wave finishes the round (every lane the same values, loop state in registers)
            RoundOut o;
            PSTAMP(4);
            finish_round_pose(A, s_tot, (int)epoch, pr, pt, chi_prev, o);
            PSTAMP(5);
            // (read here, after the solve: hoisted to the combine's loads it measured no faster,
            // DESIGN.md Appendix A "s_tmo read early")
            if (s_tmo) o.done = 1;  // a sweep timed out
            // ---- publish the new pose (and the done flag): lane l < 16 owns word l ----
            unsigned pw[PICP_POSE_GRAN];
#pragma unroll
            for (int i = 0; i < 9; ++i) pw[i] = __float_as_uint(pr[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) pw[9 + i] = __float_as_uint(pt[i]);
            pw[12] = (unsigned)o.done;
            pw[13] = my_xcc;
            pw[14] = pw[15] = 0u;
            const float w = __uint_as_float(lane_word16(pw, lane));
            if (lane < PICP_POSE_GRAN) {
              const unsigned long long gw = granule(tbase + epoch, w);
              __hip_atomic_store(pose_l2 + lane, gw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_store(pose_gl + lane, gw, RLX_AGENT);
            }
            PSTAMP(8);
            if (lane == 0) {
#pragma unroll
              for (int i = 0; i < 9; ++i) s_pose[i] = pr[i];
#pragma unroll
              for (int i = 0; i < 3; ++i) s_pose[9 + i] = pt[i];
              s_done = o.done;
              if (o.done && leader) {
                store_state(st_out + p, pr, pt, chi_prev, o, (int)epoch);
                // every block of the problem read tbase before publishing round 1, and this is
                // after its last round: the next launch's tags start past this one's
                __hip_atomic_store(tbase_p, tbase + epoch, RLX_AGENT);
              }
            }
          }
        }
      }
      __syncthreads();
      PSTAMP(3);
      // A solver has no poll in flight.  Defined here, the follower's poll state is dead on this
      // path and does not merge with it at the bottom of the round: merged, the compiler copied
      // the in-flight poll's registers on the follower's back edge and waited for the poll first.
      pa = pb = pose_sink = 0;
      if constexpr (RINGED) {
#pragma unroll
        for (int k = 0; k < RING; ++k) ring[k] = 0;
      }
    } else {
      // ---- 3. wait for the leader's pose of this round (one wave, 16 lanes) ----
      if (wave == 0) {
        unsigned long long gp = 0;
        // Polls in flight, staggered when they are first issued (two, PICP_POSE_STAGGER x 64 clocks
        // apart; with one item per lane the ring below): each poll is re-issued as soon as it has
        // been checked, so they keep their offset.  Every lane loads (lanes >= 16 repeat granule
        // 15), so a wait counts exactly one poll; the polls still in flight at the exit keep their
        // registers until the next round's wait consumes them (pose_sink), so nothing waits on
        // them: the poll state stays in the same registers round the loop (the solver path
        // redefines it, above), the slice loads are retired before the loop, and last round's
        // polls are folded into pose_sink before this round's first poll is issued (the empty asm
        // pins the fold there: sunk below the spin, it would wait for the new poll).
        // profiles/r11/waits/ and profiles/r16/pose_polls/ have the back edge as compiled.
        const int gl = lane < PICP_POSE_GRAN ? lane : PICP_POSE_GRAN - 1;
        // sc1 loads either way: past the L1, served by the L2 (the L2 copy's line stays there)
        const gu64_t* src = s_l2 ? pose_l2 : pose_gl;
        auto poll = [&]() -> unsigned long long { return __hip_atomic_load(src + gl, RLX_AGENT); };
        auto good = [&](unsigned long long v) { return __all((unsigned)(v >> 32) == tbase + epoch); };
#ifdef PICP_STAMPS
        if (epoch == 11 || epoch == 12) {  // one poll's round trip, where no pose can be there yet
          PSTAMP_VAL(11, (unsigned long long)s_l2);
          asm volatile("" ::: "memory");
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the stamp's store is out of the way
          const unsigned long long t_issue = __builtin_amdgcn_s_memrealtime();
          asm volatile("" ::: "memory");
          unsigned long long probe = poll();
          asm volatile("" : "+v"(probe)::"memory");
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the probe is back
          asm volatile("" ::: "memory");
          const unsigned long long t_back = __builtin_amdgcn_s_memrealtime();
          PSTAMP_VAL(9, t_issue);
          PSTAMP_VAL(10, t_back);
        }
#endif
        bool tmo = false;
        if constexpr (RINGED) {
          // The ring: PICP_POSE_POLLS polls in flight, PICP_POSE_SPACING x 64 clocks apart, so a
          // pose that lands in the L2 is met by the next poll to arrive there, a PICP_POSE_POLLS-th
          // of a round trip later at the most.  Polls return in the order they were issued, so
          // checking the oldest waits for exactly that one; it is re-issued at once.  The deadline
          // is read once per trip round the ring.
          // Once the pose is found the trip's remaining checks (their waits) are skipped but not
          // its remaining polls: issued on every path, they leave the registers in one order of
          // ages (ring[0] oldest) however the trip ended.  As compiled, every way out of the loop
          // meets its back edge in one block, and the compiler's wait for a check counts for the
          // youngest age the register has on any path to it: with the polls inside the branches the
          // trip's first check waited for all but one poll (s_waitcnt vmcnt(1) for
          // vmcnt(PICP_POSE_POLLS - 1)) and the ring went out in bursts.  The extra polls cost an
          // issue slot each and land unused.
#pragma unroll
          for (int k = 0; k < RING; ++k) pose_sink ^= ring[k];  // last round's polls: long complete
          asm volatile("" : "+v"(pose_sink));
#pragma unroll
          for (int k = 0; k < RING; ++k) {
            ring[k] = poll();
            if (k < RING - 1) __builtin_amdgcn_s_sleep(PICP_POSE_SPACING);
          }
          for (;;) {
            bool found = false;
#pragma unroll
            for (int k = 0; k < RING; ++k) {
              if (!found) {
                asm volatile("" : "+v"(ring[k]));  // the wait for this poll stays behind the test
                if (good(ring[k])) {
                  found = true;
                  gp = ring[k];
                }
              }
              ring[k] = poll();
            }
            if (found) break;
            if (timed_out(deadline)) { tmo = true; break; }
          }
        } else {
          pose_sink ^= pa ^ pb;  // last round's polls: long complete
          asm volatile("" : "+v"(pose_sink));
          pa = poll();
          __builtin_amdgcn_s_sleep(PICP_POSE_STAGGER);
          for (;;) {
            pb = poll();
            if (good(pa)) { gp = pa; break; }
            pa = poll();
            if (good(pb)) { gp = pb; break; }
            if (timed_out(deadline)) { tmo = true; break; }
          }
        }
        if (tmo) {
          if (lane == 0) __hip_atomic_store(errw, 2u, RLX_AGENT);
          gp = lane == 12 ? 1u : 0u;  // force done
          if (lane < 12) gp = __float_as_uint(s_pose[lane]);
        }
        // lane l stores control word l: the pose (0-11), the done flag (12), and for the solver's
        // XCC id (13) whether it is this XCD's: from the next round on, poll the L2 copy then
        const unsigned cw = lane == 13 ? (((unsigned)gp == my_xcc) ? 1u : 0u) : (unsigned)gp;
        if (lane < 14) s_ctl[lane] = cw;
      }
      __syncthreads();
      PSTAMP(2);
      PSTAMP_W1(7);
    }
  }
  // an opaque never-true test keeps the follower's last in-flight poll alive to here
  if constexpr (RINGED) {
    unsigned long long left = pose_sink;
#pragma unroll
    for (int k = 0; k < RING; ++k) left ^= ring[k];
    if (timeout_ticks == ~0ull && left == 1ull) s_pose[0] = 0.0f;
  } else {
    if (timeout_ticks == ~0ull && (pose_sink ^ pa ^ pb) == 1ull) s_pose[0] = 0.0f;
  }
}

#ifdef PICP_STAMPS
extern "C" hipError_t picp_debug_pstamps(unsigned long long* out, size_t n_words) {
  const size_t cap = sizeof(picp_pstamps) / sizeof(unsigned long long);
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(picp_pstamps), (n_words < cap ? n_words : cap) * 8, 0,
                             hipMemcpyDeviceToHost);
}
extern "C" hipError_t picp_debug_sweepstamps(unsigned long long* out, size_t n_words) {
  const size_t cap = sizeof(picp_sweepstamps) / sizeof(unsigned long long);
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(picp_sweepstamps), (n_words < cap ? n_words : cap) * 8, 0,
                                     hipMemcpyDeviceToHost);
  if (e == hipSuccess) {  // clear for the next run (a shorter sweep leaves no stale passes)
    static const unsigned long long zero[sizeof(picp_sweepstamps) / sizeof(unsigned long long)] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(picp_sweepstamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
  }
  return e;
}
#endif

// ------------------------------- host launch wrapper -------------------------------
extern "C" int picp_persistent_block(void) { return PICP_PBLOCK; }

template <int N>
static const void* persistent_kernel_n(int var) {
  switch (var) {
    case PICP_V_PINHOLE: return (const void*)picp_persistent_kernel<N, PICP_V_PINHOLE, PICP_PBLOCK>;
    case PICP_V_PINHOLE_KEEP: return (const void*)picp_persistent_kernel<N, PICP_V_PINHOLE_KEEP, PICP_PBLOCK>;
    default: return (const void*)picp_persistent_kernel<N, PICP_V_GENERAL, PICP_PBLOCK>;
  }
}

// Blocks of the persistent variant for (npt, K) one CU holds at once (registers, LDS, waves).
// Its blocks hand rounds to each other, so the host launches it only when grid <= this x CUs.
extern "C" hipError_t picp_persistent_occupancy(int npt, const float K[9], int* blocks_per_cu) {
  if (!blocks_per_cu) return hipErrorInvalidValue;
  // the smaller of the two pinhole variants: keep_outliers is a per-solve argument
  int best = -1;
  for (int keep = 0; keep < 2; ++keep) {
    const void* fn = nullptr;
    switch (npt) {
      case 1: fn = persistent_kernel_n<1>(picp_variant(K, keep)); break;
      case 2: fn = persistent_kernel_n<2>(picp_variant(K, keep)); break;
      case 4: fn = persistent_kernel_n<4>(picp_variant(K, keep)); break;
      case 8: fn = persistent_kernel_n<8>(picp_variant(K, keep)); break;
      default: return hipErrorInvalidValue;
    }
    int occ = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, PICP_PBLOCK, 0);
    if (e != hipSuccess) return e;
    best = (best < 0 || occ < best) ? occ : best;
  }
  *blocks_per_cu = best;
  return hipSuccess;
}

extern "C" hipError_t picp_launch_persistent(hipStream_t stream, int grid, int npt, const float* X,
                                             const float* Y, const float* Z, const float* U,
                                             const float* V, const PicpArgs* args,
                                             const PicpState* st_in, PicpState* st_out,
                                             unsigned long long* gpart, unsigned long long* gpose,
                                             unsigned int* err, unsigned int* tagbase,
                                             unsigned long long timeout_ticks) {
  if (grid <= 0 || !args || !args->uniform || args->nblk_u > PICP_MAX_PBLK) return hipErrorInvalidValue;
  // PICP_SWEEP_LAG_NS (read once; for tests and measurements): the lag of the solvers' first sweep
  // pass, 0 = straight after the barrier, at most 100 us.  A problem whose blocks are all solvers
  // has no follower to wait for: they publish as they leave the barrier, so no lag there.
  static const unsigned long long sweep_lag = [] {
    const char* e = getenv("PICP_SWEEP_LAG_NS");
    long ns = e ? atol(e) : PICP_SWEEP_LAG_NS_DEFAULT;
    ns = ns < 0 ? 0 : (ns > 100000 ? 100000 : ns);
    return (unsigned long long)((ns + 5) / 10);  // s_memrealtime ticks
  }();
  const int var = picp_variant(args->K, args->keep_outliers);
#define PICP_LAUNCH_PV(N, PV)                                                                       \
  hipLaunchKernelGGL((picp_persistent_kernel<N, PV, PICP_PBLOCK>), dim3(grid), dim3(PICP_PBLOCK), 0, \
                     stream, X, Y, Z, U, V, *args, st_in, st_out, gpart, gpose, err, tagbase,         \
                     args->nblk_u > PICP_PSOLVERS ? sweep_lag : 0ull, timeout_ticks)
#define PICP_LAUNCH_P(N)                                                            \
  if (var == PICP_V_PINHOLE) PICP_LAUNCH_PV(N, PICP_V_PINHOLE);                     \
  else if (var == PICP_V_PINHOLE_KEEP) PICP_LAUNCH_PV(N, PICP_V_PINHOLE_KEEP);      \
  else PICP_LAUNCH_PV(N, PICP_V_GENERAL)
  switch (npt) {
    case 1: PICP_LAUNCH_P(1); break;
    case 2: PICP_LAUNCH_P(2); break;
    case 4: PICP_LAUNCH_P(4); break;
    case 8: PICP_LAUNCH_P(8); break;
    default: return hipErrorInvalidValue;
  }
#undef PICP_LAUNCH_P
#undef PICP_LAUNCH_PV
  return hipGetLastError();
}
