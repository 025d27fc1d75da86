// refine.hip -- best-move refinement of a commit's hunk groups (hdg_refine, include/hdgnn.h):
// local search on the correlation-clustering objective the linkages approximate, from any
// starting partition.  The definitions (fixed-point gains, start, sweep, tie rules, outputs)
// are the header's; every result is an integer and independent of summation order.
//
// Two launches, neither waits for another block:
//   k_rf_weights  grid (ut_tiles(nc), B), 512 threads: the staging of the I x J segment of the
//                 scores and its mirror through two 64 x 65 LDS tiles (ut_stage), one tile pair
//                 per block.  Every p < q of the tile (ut_visit) gets its weight (ut_weight)
//                 and from it the gain a_pq = rint(clamp(w - t') * 2^18), 0 for a pair that is
//                 no edge.
//                 The commit's region of the workspace holds the full nc x nc int32 matrix,
//                 written at (p, q) by rows of the segment and, through the second LDS tile,
//                 at (q, p) by rows of the mirror: both stores are row-coalesced, and the
//                 sweep reads a hunk's whole row contiguously.  The diagonal is written as 0.
//                 The block's count of pairs that are no edge follows the matrix.
//   k_rf_sweep    grid B, 1024 threads (thread h owns hunk h and slot h, and h + 1024 above
//                 1024).  Slots, slot sizes and two buffers of per-slot sums live in LDS; a
//                 thread keeps its own hunks' slots in registers.  The step over p is
//                 sequential.  A step: every q adds a_pq (row p of the workspace matrix,
//                 loaded one step ahead) into S[slot[q]] with an int32 LDS atomicAdd; barrier;
//                 every non-empty slot h != g offers (S[h], h), every empty one (0, h) if p is
//                 not alone, packed into one 64-bit key whose maximum is the header's choice
//                 (value, then non-empty before empty, then the lowest slot): wave maxima by
//                 DPP, the other buffer of sums is zeroed for the next step; barrier;
//                 every thread reads the wave maxima and reaches the same decision, the
//                 owner of p and thread 0 apply it.  Two barriers per step; what a step
//                 writes is read only after the next step's first barrier.  The sweep loop is
//                 bounded by max_sweeps, the step loop by nc, every inner loop by nc.  Then
//                 the final slots and the label graph are labelled (ut_label, ut_true_groups),
//                 the pairs counted (ut_pair_counts, ut_pair_table), and groups, ut and rq
//                 written.
//
// hdg_refine_ladder is the same two kernel bodies, each stated once (rf_weights, rf_sweep):
//   k_rl_weights  rf_weights storing the fp32 weight of a pair instead of its gain at one
//                 bound; one canonical NaN for a pair that is no edge and on the diagonal.
//   k_rl_sweep    rf_sweep on a grid (rungs, B), the rung on blockIdx.x: a matrix word becomes
//                 a gain by rf_gain on the stored w against the rung's bound (hdg_refine's
//                 bits: the same function of the same w), the bounds a by-value argument.  The
//                 start is the tree's cut at the rung: k_cut's unions (ut_union, levels > t'
//                 strictly, rows of -1 / NaN skipped) and ut_label in the LDS arrays of the
//                 sums, which are free before the sweeps; bounded by nc - 1.
//
// hdg_refine_merge and hdg_refine_merge_ladder are those sweep blocks with rounds
// (rf_sweep<LADDER, MERGE = true>, k_rm_sweep and k_rml_sweep; the weights launches are the two
// above): a round is the node phase -- the sweeps above, unchanged -- and one group sweep, which
// lets two whole groups merge.  A group sweep inside the block:
//   chains   once per group sweep every slot's members are chained through first (a slot's
//            head), g (a member's successor) and t (a slot's tail), which are free between the
//            start and the final labelling: one LDS exchange per hunk.  A merge appends one
//            chain to another in O(1) (thread 0).  The order of a chain does not matter: every
//            sum is an integer.
//   visit g  every thread sums a_pq over the members p of g for its own hunks q in registers
//            (int32: at most UT_MAXN - 1 members), reading the members' rows from the workspace
//            one member ahead; no barrier between rows.  Then C[h] = sum of c_q over q in h by
//            two int32 LDS atomics on a 16-bit split of c_q (low parts into S[0], high parts
//            into S[1]: exact, UT_MAXN * 2^16 < 2^31); barrier; every owner of a non-empty slot
//            h != g offers rm_key(C[h], h) and zeroes its two sums, wave maxima by rf_wave_max;
//            barrier; every thread reaches the same decision and rewrites its own hunks' slots,
//            thread 0 the sizes and the chain.  Two barriers per non-empty slot, none for an
//            empty one: what thread 0 writes after a merge belongs to slots min(g, h) <= g
//            and max(g, h), and the visits up to the next barrier read neither (the emptied
//            slot is skipped from a register).
// The round loop is bounded by max_rounds, a group sweep's visits by nc, a chain walk by the
// slot's size, the total of node sweeps by max_sweeps.
//
// hdg_refine_split and hdg_refine_split_ladder are the sweep blocks with rounds whose sweeps a
// runtime `kinds` chooses (rf_sweep<LADDER, RF_SPLIT>, k_rs_sweep and k_rsl_sweep; the weights
// launches are again the two above): after the node phase the group sweep above, a split sweep,
// or one after the other.  A split sweep inside the block (rs_split_sweep), in the LDS arrays
// the chains use (first, g, t), so no LDS is added:
//   visit g  skipped without a barrier if g holds fewer than 2 hunks or a split of this sweep
//            filled it (one flag per slot).  The members are compacted in index order (a
//            ballot per wave and owned hunk, the waves' counts through LDS).  Seeds: one walk
//            over the members' rows, every thread keeping the smallest rs_key (gain, p, q) of
//            its own columns in g; the block minimum through rf_wave_max on the complement.
//   a step   one member m of a pass: row m, read one member ahead, restricted to the columns
//            in g; each thread adds the gains of its own hunks to T_G or T_E by the side it
//            holds for them in a register; wave sums, then one int32 LDS atomic per wave and
//            side into one of three small buffers used in turn; m's owner puts m's side beside
//            them; ONE barrier; every thread reads the three words and reaches the same
//            decision, m's owner records it, and every thread carries C and the size of side
//            E along.  Thread 0 zeroes the buffer of the step after the next: its readers are
//            before this step's barrier and its adders behind the next step's.
//   the cut  if C < 0: the smallest empty slot by a block maximum of keys; every thread
//            rewrites the slots of its own hunks on side E, thread 0 the two sizes and the flag.
// A split sweep's visits are bounded by nc, the passes by HDG_RS_PASSES, a pass's steps by the
// slot's size; every index read from LDS is range-checked before it addresses anything.
// Integer results only; the same bits on every run.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

using hdg::fail;
typedef unsigned long long u64;

constexpr int RF_NT = UT_CLOSE_NT;
constexpr int RF_WAVES = RF_NT / 64;
constexpr float RF_SCALE = 262144.f;         // 2^18: a = rint(d * 2^18), |a| <= 2^19
static_assert(RF_NT * UT_PER == UT_MAXN, "a thread owns UT_PER hunks and slots");
static_assert((UT_MAXN - 1) * (1ll << 19) < (1ll << 31), "a node sum fits int32");
static_assert(UT_MAXN <= 2048, "the key's tie field holds two ranges of 2048 slots");
// a group sweep (hdg_refine_merge): the gain of a merge and its key, the 16-bit split
static_assert((long long)(UT_MAXN / 2) * (UT_MAXN / 2) * (1ll << 19) <= (1ll << 39),
              "a merge gain is at most 2^39 in magnitude");
static_assert(UT_MAXN <= (1 << 11), "the merge key's tie field holds 11 bits of slot");
static_assert(41 + 11 <= 64, "the biased merge gain (below 2^41) and the tie field fit one key");
static_assert((long long)UT_MAXN * (1ll << 16) < (1ll << 31), "a slot's sum of 16-bit parts fits int32");
// a split sweep (hdg_refine_split): a side sum, the sum between the sides, the seed key
static_assert((UT_MAXN - 1) * (1ll << 19) < (1ll << 31), "a side sum fits int32");
static_assert((long long)(UT_MAXN / 2) * (UT_MAXN / 2) * (1ll << 19) <= (1ll << 39),
              "the sum between the two sides is at most 2^39 in magnitude");
static_assert(21 + 11 + 11 < 64, "the biased gain (21 bits) and two hunk indices fit one seed key");
static_assert(HDG_RS_Q_SLOTS == HDG_RM_Q_SLOTS && HDG_RS_Q_SPLITS == HDG_RM_Q_SLOTS - 1,
              "hdg_refine_split's rq row is hdg_refine_merge's with the last slot in use");
static_assert(HDG_RS_PASSES >= 1, "a split attempt has its assignment pass");

// workspace, in 4-byte words per commit: the nc x nc matrix of gains, then ut_tiles(nc)
// no-edge counts, rounded up to an even number of words
__host__ __device__ inline size_t rf_commit_words(const int nc) {
  return ((size_t)nc * (size_t)nc + (size_t)ut_tiles(nc) + 1) & ~(size_t)1;
}

// the fixed-point gain of a pair of weight w against the link bound tp (finite)
__device__ __forceinline__ int32_t rf_gain(const float w, const float tp) {
  const float d = w - tp;
  return (int32_t)rintf(fminf(fmaxf(d, -2.f), 2.f) * RF_SCALE);
}

// The canonical word of a pair that is no edge in the matrix of weights (hdg_refine_ladder):
// one quiet NaN.  ut_weight never returns a NaN weight for an edge.
constexpr int32_t RL_NONE = 0x7FC00000;

// what the matrix holds for a pair: hdg_refine's gain against the one bound of the call ...
struct rf_as_gain {
  float tp;
  __device__ __forceinline__ int32_t operator()(const bool edge, const float w) const {
    return edge ? rf_gain(w, tp) : 0;
  }
};
// ... or the fp32 weight itself, for every rung of hdg_refine_ladder to form its gain from
struct rl_as_weight {
  __device__ __forceinline__ int32_t operator()(const bool edge, const float w) const {
    return edge ? __float_as_int(w) : RL_NONE;
  }
};

// The weights kernel of both entry points: staging, the pass by rows of the segment and the
// pass by rows of the mirror, the no-edge count.  `word` says what is stored for a pair
// (edge, w); the diagonal holds the word of a pair that is no edge.
template <class Word>
__device__ __forceinline__ void rf_weights(const float* __restrict__ probs,
                                           int32_t* __restrict__ ws, const int nc, const int rule,
                                           const Word word) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a), then the word's bits
  __shared__ uint32_t red[UT_LINK_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  int p0, q0;                              // this block's tile pair
  ut_tile_pair((int)blockIdx.x, nc, p0, q0);
  ut_stage(ut_scores(probs, b, nc), nc, p0, q0, sa, sb);
  __syncthreads();
  int32_t* wb = ws + (size_t)b * rf_commit_words(nc);
  uint32_t nans = 0;
  ut_visit(nc, p0, q0, sa, sb,             // only this thread reads or writes sb[c][a]
           [&](int, const int a, const int c, const int p, const int q, const float spq,
               const float sqp) {
             float w;
             const bool edge = ut_weight(rule, spq, sqp, w);
             if (!edge) ++nans;
             const int32_t g = word(edge, w);
             wb[(size_t)p * nc + q] = g;
             sb[c * UT_LD + a] = __int_as_float(g);
           });
  if (p0 == q0 && tid < UT_T && p0 + tid < nc)
    wb[(size_t)(p0 + tid) * (nc + 1)] = word(false, 0.f);                                 // (p, p)
  __syncthreads();
  ut_visit<true>(nc, p0, q0, sa, sb,       // by rows of the mirror: (q, p) for the p < q above
                 [&](int, int, int, const int p, const int q, float, const float gqp) {
                   wb[(size_t)q * nc + p] = __float_as_int(gqp);
                 });
  ut_count_put(red, nans);
  __syncthreads();
  if (tid == 0)
    reinterpret_cast<uint32_t*>(wb)[(size_t)nc * nc + blockIdx.x] =
        ut_count_sum<uint32_t, UT_LINK_WAVES>(red, 0);
}

__global__ __launch_bounds__(UT_LINK_NT) void k_rf_weights(const float* __restrict__ probs,
                                                           int32_t* __restrict__ ws, const int nc,
                                                           const int rule, const float tp) {
  rf_weights(probs, ws, nc, rule, rf_as_gain{tp});
}

__global__ __launch_bounds__(UT_LINK_NT) void k_rl_weights(const float* __restrict__ probs,
                                                           int32_t* __restrict__ ws, const int nc,
                                                           const int rule) {
  rf_weights(probs, ws, nc, rule, rl_as_weight{});
}

// a candidate of a step as one key: the larger key wins.  Value, then a non-empty slot
// before an empty one, then the lower slot.  0 is no candidate (|v| < 2^30).
__device__ __forceinline__ u64 rf_key(const int32_t v, const bool empty, const int h) {
  return ((u64)((uint32_t)v ^ 0x80000000u) << 12) | (u64)((empty ? 0 : 2048) + (2047 - h));
}

// a candidate of a group visit as one key: the larger key wins.  The gain C (|C| <= 2^39,
// biased by 2^40: never 0), then the lower slot.  0 is no candidate.
constexpr long long RM_BIAS = 1ll << 40;
__device__ __forceinline__ u64 rm_key(const long long c, const int h) {
  return ((u64)(c + RM_BIAS) << 11) | (u64)(2047 - h);
}

// max(k, the key CTRL brings from another lane); a lane without a source, or in a row ROWS
// masks out, gets 0, the identity
template <int CTRL, int ROWS>
__device__ __forceinline__ u64 rf_dpp_max(const u64 k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, ROWS, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, ROWS,
                                                            0xF, false);
  const u64 other = ((u64)hi << 32) | lo;
  return other > k ? other : k;
}

// the wave's largest key, in lane 63: DPP in the VALU, no LDS round trips
__device__ __forceinline__ u64 rf_wave_max(u64 k) {
  k = rf_dpp_max<0x111, 0xF>(k);           // row_shr:1
  k = rf_dpp_max<0x112, 0xF>(k);           // row_shr:2
  k = rf_dpp_max<0x114, 0xF>(k);           // row_shr:4
  k = rf_dpp_max<0x118, 0xF>(k);           // row_shr:8: lane 15 of a row holds the row's
  k = rf_dpp_max<0x142, 0xA>(k);           // row_bcast:15 into rows 1 and 3
  k = rf_dpp_max<0x143, 0xC>(k);           // row_bcast:31 into rows 2 and 3
  return k;
}

__device__ __forceinline__ long long rf_wave_sum64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the bounds of a ladder's rungs, a by-value kernel argument
struct rl_bounds {
  float tp[HDG_RL_MAX_RUNGS];
};

// a word of the matrix as a gain: hdg_refine's matrix holds the gain; the ladder's holds the
// weight, and rf_gain on the same w against the rung's bound is hdg_refine's gain bit for bit
template <bool LADDER>
__device__ __forceinline__ int32_t rf_word_gain(const int32_t word, const float tp) {
  if constexpr (!LADDER) return word;
  const float w = __int_as_float(word);
  return w != w ? 0 : rf_gain(w, tp);
}

// One group sweep of hdg_refine_merge inside the sweep block (the header's definition; the
// steps at the top of this file), after a node phase: the last step's move is not yet behind
// a barrier, S[cur] is zero and the other buffer is not.  head, next and tail are the block's
// first, g and t.  my: this thread's hunks' slots, rewritten by a merge.  -> the merges made,
// uniform; their gains are added to `gain`.  On return both buffers of S are zero and every
// write is behind a barrier.
template <bool LADDER>
__device__ __forceinline__ uint32_t rm_group_sweep(const int32_t* __restrict__ wb, const float tp,
                                                   const int nc, const int nwav,
                                                   int32_t (*S)[UT_MAXN], int32_t* slot,
                                                   int32_t* size, int32_t* head, uint32_t* next,
                                                   uint32_t* tail, u64* wkey,
                                                   int32_t (&my)[UT_PER], long long& gain) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    if (i < nc) {
      head[i] = -1;
      S[0][i] = S[1][i] = 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {       // a slot's chain: the last to arrive is its head,
    const int i = tid + u * RF_NT;         // the first its tail
    if (i < nc) {
      const int32_t old = atomicExch(&head[my[u]], i);
      next[i] = (uint32_t)old;
      if (old < 0) tail[my[u]] = (uint32_t)i;
    }
  }
  __syncthreads();

  uint32_t merged = 0;
  int emptied = -1;                        // the slot the last merge emptied: its size may not
  for (int gv = 0; gv < nc; ++gv) {        // be behind a barrier yet
    const int sz = size[gv];
    if (sz <= 0 || gv == emptied) continue;                 // uniform
    // c_q = the sum of a_pq over the members p of gv, for this thread's q
    int32_t c[UT_PER], pre[UT_PER];
    uint32_t m = (uint32_t)head[gv];
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int q = tid + u * RF_NT;
      c[u] = 0;
      pre[u] = (m < (uint32_t)nc && q < nc) ? wb[(size_t)m * nc + q] : 0;
    }
    for (int k = 0; k < sz && m < (uint32_t)nc; ++k) {      // sz <= nc: a chain cannot spin
      const uint32_t mn = next[m];
      const bool more = k + 1 < sz && mn < (uint32_t)nc;
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        c[u] += rf_word_gain<LADDER>(pre[u], tp);
        pre[u] = (more && q < nc) ? wb[(size_t)mn * nc + q] : 0;      // the next member's row
      }
      m = mn;
    }
    // C[h] = the sum of c_q over q in h: low 16 bits into S[0], the rest into S[1]
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int q = tid + u * RF_NT;
      if (q < nc && my[u] != gv && c[u] != 0) {
        atomicAdd(&S[0][my[u]], c[u] & 0xFFFF);
        atomicAdd(&S[1][my[u]], c[u] >> 16);
      }
    }
    __syncthreads();
    if (wave < nwav) {
      u64 key = 0;
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int h = tid + u * RF_NT;
        if (h < nc) {
          if (h != gv && size[h] > 0) {
            const u64 k = rm_key((long long)S[1][h] * 65536 + (long long)S[0][h], h);
            key = k > key ? k : key;
          }
          S[0][h] = S[1][h] = 0;           // for the next visit
        }
      }
      key = rf_wave_max(key);
      if (lane == 63) wkey[wave] = key;
    }
    __syncthreads();
    u64 best = 0;
    for (int w = 0; w < nwav; ++w) best = wkey[w] > best ? wkey[w] : best;
    const long long val = (long long)(best >> 11) - RM_BIAS;
    if (best != 0 && val > 0) {            // uniform: every thread holds the same decision
      const int h = 2047 - (int)(best & 2047u);
      const int to = h < gv ? h : gv, from = h < gv ? gv : h;
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int i = tid + u * RF_NT;
        if (i < nc && my[u] == from) {
          my[u] = to;
          slot[i] = to;
        }
      }
      if (tid == 0) {                      // the chain of `from` goes behind the chain of `to`
        const uint32_t end = tail[to];
        if (end < (uint32_t)nc) next[end] = (uint32_t)head[from];
        tail[to] = tail[from];
        size[to] += size[from];
        size[from] = 0;
      }
      emptied = from;
      ++merged;
      gain += val;
    }
  }
  __syncthreads();
  return merged;
}

// a seed pair of a split visit as one key: the smaller key wins.  The gain a_pq (|a| <= 2^19,
// biased by 2^19 into 21 bits), then the lower p, then the lower q.  Below 2^43, so the
// complement a block maximum goes through is never 0.
constexpr int32_t RS_BIAS = 1 << 19;
__device__ __forceinline__ u64 rs_key(const int32_t a, const int p, const int q) {
  return ((u64)(uint32_t)(a + RS_BIAS) << 22) | ((u64)p << 11) | (u64)q;
}

__device__ __forceinline__ int32_t rs_wave_sum32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the block's largest key, in every thread: wave maxima by rf_wave_max, all waves through wkey,
// which is free on entry and again on return
__device__ __forceinline__ u64 rs_block_max(u64 key, u64* wkey) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  key = rf_wave_max(key);
  if (lane == 63) wkey[wave] = key;
  __syncthreads();
  u64 best = 0;
  for (int w = 0; w < RF_WAVES; ++w) best = wkey[w] > best ? wkey[w] : best;
  __syncthreads();
  return best;
}

// One split sweep of hdg_refine_split inside the sweep block (the header's definition), after
// a node phase or a group sweep: what they wrote need not be behind a barrier yet, and the two
// buffers of S are left as they are.  mem, filled and scr are the block's first, g and t:
//   mem      the members of the visited slot, compacted in index order (ballots, wave counts)
//   filled   per slot: 1 if a split of this sweep filled it
//   scr      words 0 .. 8: three buffers of (T_G, T_E, the side of m), used in turn by the
//            steps -- a step adds into buffer st % 3, and after its one barrier thread 0 zeroes
//            buffer (st + 2) % 3, whose last readers are before that barrier and whose next
//            adders are behind the next one; words 16 .. 16 + UT_PER * RF_WAVES: the counts
//            of the compaction
// A thread keeps the sides of its own hunks in registers (0 not a member or not yet assigned,
// 1 side G, 2 side E); the side of the step's member m reaches the block through the step's
// buffer.  C, the sum between the sides, is carried by every thread.  my: this thread's hunks'
// slots, rewritten by a split.  -> the splits made, uniform; their gains are added to `gain`.
// On return every write is behind a barrier.
template <bool LADDER>
__device__ __forceinline__ uint32_t rs_split_sweep(const int32_t* __restrict__ wb, const float tp,
                                                   const int nc, int32_t* slot, int32_t* size,
                                                   int32_t* mem, uint32_t* filled, uint32_t* scr,
                                                   u64* wkey, int32_t (&my)[UT_PER],
                                                   long long& gain) {
  constexpr int CNT = 16;                  // where the compaction's counts start in scr
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* acc = reinterpret_cast<int32_t*>(scr);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    if (i < nc) filled[i] = 0;
  }
  if (tid < 9) acc[tid] = 0;
  __syncthreads();

  uint32_t splits = 0;
  uint32_t st = 0;                         // steps made: the buffer of a step is st % 3
  for (int gv = 0; gv < nc; ++gv) {
    const int n = size[gv];
    if (n < 2 || n > nc || filled[gv] != 0) continue;       // uniform
    // ---- the members of gv in index order ---------------------------------------------------
    bool in[UT_PER];
    u64 bal[UT_PER];
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int i = tid + u * RF_NT;
      in[u] = i < nc && my[u] == gv;
      bal[u] = __ballot(in[u]);
      if (lane == 0) scr[CNT + u * RF_WAVES + wave] = (uint32_t)__popcll(bal[u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {     // a member's place: the members before it
      if (!in[u]) continue;
      uint32_t off = (uint32_t)__popcll(bal[u] & ((1ull << lane) - 1ull));
      for (int w = 0; w < u * RF_WAVES + wave; ++w) off += scr[CNT + w];
      if (off < (uint32_t)nc) mem[off] = tid + u * RF_NT;
    }
    __syncthreads();

    // ---- seeds: the smallest a_pq over p < q in gv, one walk over the members' rows ---------
    u64 kmin = ~0ull;
    {
      uint32_t m = (uint32_t)mem[0];
      int32_t pre[UT_PER];
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        pre[u] = (m < (uint32_t)nc && in[u]) ? wb[(size_t)m * nc + q] : 0;
      }
      for (int k = 0; k < n && m < (uint32_t)nc; ++k) {
        const uint32_t mn = k + 1 < n ? (uint32_t)mem[k + 1] : (uint32_t)nc;
#pragma unroll
        for (int u = 0; u < UT_PER; ++u) {
          const int q = tid + u * RF_NT;
          if (in[u] && q > (int)m) {
            const u64 key = rs_key(rf_word_gain<LADDER>(pre[u], tp), (int)m, q);
            kmin = key < kmin ? key : kmin;
          }
          pre[u] = (mn < (uint32_t)nc && in[u]) ? wb[(size_t)mn * nc + q] : 0;
        }
        m = mn;
      }
    }
    const u64 seed = ~rs_block_max(~kmin, wkey);
    const int32_t a12 = (int32_t)(uint32_t)(seed >> 22) - RS_BIAS;
    if (seed == ~0ull || a12 >= 0) continue;                // uniform: no cut of gv can raise Q
    const int s1 = (int)((seed >> 11) & 2047u), s2 = (int)(seed & 2047u);
    int32_t sd[UT_PER];
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int i = tid + u * RF_NT;
      sd[u] = i == s1 ? 1 : (i == s2 ? 2 : 0);
    }
    long long C = a12;
    int nE = 1;

    // ---- the assignment pass, then the correction passes ------------------------------------
    for (int pass = 0; pass < HDG_RS_PASSES; ++pass) {
      bool changed = false;
      uint32_t m = (uint32_t)mem[0];
      int32_t pre[UT_PER];
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        pre[u] = (m < (uint32_t)nc && in[u]) ? wb[(size_t)m * nc + q] : 0;
      }
      for (int k = 0; k < n && m < (uint32_t)nc; ++k) {
        const uint32_t mn = k + 1 < n ? (uint32_t)mem[k + 1] : (uint32_t)nc;
        int32_t tg = 0, te = 0, mine = 0;
#pragma unroll
        for (int u = 0; u < UT_PER; ++u) {
          const int q = tid + u * RF_NT;
          const int32_t a = rf_word_gain<LADDER>(pre[u], tp);
          pre[u] = (mn < (uint32_t)nc && in[u]) ? wb[(size_t)mn * nc + q] : 0;   // the next row
          if (q == (int)m) mine = sd[u];   // a_mm is 0: m adds nothing to its own side
          else if (sd[u] == 1) tg += a;
          else if (sd[u] == 2) te += a;
        }
        const bool is_seed = (int)m == s1 || (int)m == s2;  // uniform
        const uint32_t at = m;
        m = mn;
        if (is_seed) continue;
        int32_t* ab = acc + 3 * (st % 3u);
        tg = rs_wave_sum32(tg);
        te = rs_wave_sum32(te);
        if (lane == 0) {
          if (tg != 0) atomicAdd(&ab[0], tg);
          if (te != 0) atomicAdd(&ab[1], te);
        }
        if (tid == (int)(at & (uint32_t)(RF_NT - 1))) ab[2] = mine;       // m's owner
        __syncthreads();
        const int32_t TG = ab[0], TE = ab[1], X = ab[2];
        if (tid == 0) {
          int32_t* az = acc + 3 * ((st + 2u) % 3u);
          az[0] = az[1] = 0;
        }
        ++st;
        int to = 0;                        // the side m takes, 0: it keeps its own
        if (pass == 0) {
          to = TE > TG ? 2 : 1;
          C += to == 2 ? TG : TE;          // the sum over the other side
          nE += to == 2;
        } else {
          const int32_t own = X == 2 ? TE : TG, other = X == 2 ? TG : TE;
          if ((X == 1 || X == 2) && other > own) {
            to = 3 - X;
            C += (long long)own - (long long)other;
            nE += to == 2 ? 1 : -1;
            changed = true;
          }
        }
        if (to != 0) {
#pragma unroll
          for (int u = 0; u < UT_PER; ++u)
            if (tid + u * RF_NT == (int)at) sd[u] = to;
        }
      }
      if (pass > 0 && !changed) break;     // uniform
    }

    // ---- the decision -----------------------------------------------------------------------
    if (C < 0) {                           // uniform
      u64 key = 0;                         // the smallest empty slot
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int h = tid + u * RF_NT;
        if (h < nc && size[h] == 0) {
          const u64 k = (u64)(UT_MAXN - h);
          key = k > key ? k : key;
        }
      }
      const u64 best = rs_block_max(key, wkey);
      if (best != 0 && nE > 0 && nE < n) { // a slot of 2 hunks leaves a slot empty
        const int e = UT_MAXN - (int)best;
#pragma unroll
        for (int u = 0; u < UT_PER; ++u) {
          const int i = tid + u * RF_NT;
          if (i < nc && sd[u] == 2) {
            my[u] = e;
            slot[i] = e;
          }
        }
        if (tid == 0) {
          size[e] = nE;
          size[gv] = n - nE;
          filled[e] = 1;
        }
        ++splits;
        gain -= C;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  return splits;
}

// The sweep block of both entry points, on one commit (and one rung): wb its matrix, yb its
// label rows, and groups (or NULL), row and qrow where its outputs go.  The start is gin, the
// commit's ids (or NULL) -- or with LADDER the cut of the commit's tree (merges, levels; or
// NULL) at tp, k_cut's unions.  gin and groups may be the same array: a commit's ids are all
// read before the first barrier and written after the last.
// With ROUNDS = RF_MERGE the sweeps are hdg_refine_merge's rounds (at most max_rounds; a node
// phase, then one group sweep) and qrow has HDG_RM_Q_SLOTS slots; with RF_SPLIT they are
// hdg_refine_split's (a node phase, then the sweeps `kinds` names: a group sweep, a split sweep);
// with RF_PLAIN neither max_rounds nor kinds is read.
constexpr int RF_PLAIN = 0, RF_MERGE = 1, RF_SPLIT = 2;
template <bool LADDER, int ROUNDS>
__device__ __forceinline__ void rf_sweep(const int32_t* __restrict__ wb,
                                         const uint32_t* __restrict__ yb, const int32_t* gin,
                                         const int32_t* __restrict__ merges,
                                         const float* __restrict__ levels, const float tp,
                                         int32_t* groups, u64* __restrict__ row,
                                         long long* __restrict__ qrow, const int nc,
                                         const int max_sweeps, const int max_rounds,
                                         const int kinds) {
  __shared__ int32_t S[2][UT_MAXN];        // the per-slot sums of this step and the next
  __shared__ int32_t slot[UT_MAXN];
  __shared__ int32_t size[UT_MAXN];
  __shared__ int32_t first[UT_MAXN];       // smallest member of a starting id / a final slot
  __shared__ uint32_t g[UT_MAXN];
  __shared__ uint32_t t[UT_MAXN];
  __shared__ u64 wkey[RF_WAVES];
  __shared__ long long wq[RF_WAVES];
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t red[UT_CLOSE_WAVES * 3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool started = gin != nullptr;           // uniform: a start other than every hunk alone

  // ---- the tree's cut at tp, as k_cut unites it: ids in g; S is free before the sweeps ------
  if constexpr (LADDER) {
    if (merges) {                          // uniform
      uint32_t* par = reinterpret_cast<uint32_t*>(S[0]);
      for (int i = tid; i < nc; i += RF_NT) par[i] = (uint32_t)i;
      __syncthreads();
      for (int k = tid; k < nc - 1; k += RF_NT) {
        const int32_t p = merges[2 * k], q = merges[2 * k + 1];
        if (levels[k] > tp && p >= 0 && q >= 0 && p < nc && q < nc)      // NaN compares false
          ut_union(par, (uint32_t)p, (uint32_t)q);
      }
      __syncthreads();
      ut_label(par, reinterpret_cast<uint32_t*>(S[1]), g, wsum, nc);
      started = true;
    }
  }

  // ---- start: a group sits in the slot of its smallest member -------------------------------
  int32_t id[UT_PER], my[UT_PER], nx[UT_PER];
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    id[u] = -1;
    nx[u] = 0;
    if (i < nc) {
      if (gin) id[u] = gin[i];
      else if (LADDER && started) id[u] = (int32_t)g[i];
      nx[u] = wb[i];                       // row 0 of the matrix, for step 0
      first[i] = 0x7FFFFFFF;
      size[i] = 0;
      S[0][i] = S[1][i] = 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    if (i < nc && (uint32_t)id[u] < (uint32_t)nc) atomicMin(&first[id[u]], i);
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    my[u] = i;
    if (i < nc) {
      if ((uint32_t)id[u] < (uint32_t)nc) my[u] = first[id[u]];
      slot[i] = my[u];
      atomicAdd(&size[my[u]], 1);
    }
  }
  __syncthreads();

  // ---- Q at the start: this thread's q against every p < q of its slot ----------------------
  long long q_start = 0;
  if (started) {                           // uniform; singletons have Q = 0
    for (int p = 0; p < nc - 1; ++p) {
      const int32_t sp = slot[p];
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        if (q > p && q < nc && my[u] == sp)
          q_start += rf_word_gain<LADDER>(wb[(size_t)p * nc + q], tp);
      }
    }
    q_start = rf_wave_sum64(q_start);
    if (lane == 0) wq[wave] = q_start;
    __syncthreads();
    q_start = 0;
    for (int w = 0; w < RF_WAVES; ++w) q_start += wq[w];
  }

  // ---- sweeps ------------------------------------------------------------------------------
  const int nwav = nc >= RF_NT ? RF_WAVES : (nc + 63) >> 6;     // the waves that own a slot
  int cur = 0, sweeps = 0, converged = 0;
  uint32_t moves = 0;
  long long gain = 0;
  int rounds = 0;                          // with rounds: those run, their merges and splits,
  uint32_t nmerged = 0, nsplit = 0;        // and the gain of the first node phase
  long long node_gain = 0;
  for (int sw = 0; sw < max_sweeps; ++sw) {
    bool moved = false;
    for (int p = 0; p < nc; ++p) {
      int32_t a[UT_PER];
      const int32_t* nrow = wb + (size_t)(p + 1 < nc ? p + 1 : 0) * nc;
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        a[u] = rf_word_gain<LADDER>(nx[u], tp);
        nx[u] = q < nc ? nrow[q] : 0;      // the next step's row
        if (q < nc && q != p && a[u] != 0) atomicAdd(&S[cur][my[u]], a[u]);
      }
      __syncthreads();
      const int gs = slot[p];
      const int32_t stay = S[cur][gs];
      const bool roomy = size[gs] > 1;
      if (wave < nwav) {
        u64 key = 0;
#pragma unroll
        for (int u = 0; u < UT_PER; ++u) {
          const int h = tid + u * RF_NT;
          if (h < nc) {
            u64 k = 0;
            if (size[h] > 0) {
              if (h != gs) k = rf_key(S[cur][h], false, h);
            } else if (roomy) {
              k = rf_key(0, true, h);
            }
            key = k > key ? k : key;
          }
        }
        key = rf_wave_max(key);
        if (lane == 63) wkey[wave] = key;
      }
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int h = tid + u * RF_NT;
        if (h < nc) S[cur ^ 1][h] = 0;
      }
      __syncthreads();
      u64 best = 0;
      for (int w = 0; w < nwav; ++w) best = wkey[w] > best ? wkey[w] : best;
      const int32_t val = (int32_t)((uint32_t)(best >> 12) ^ 0x80000000u);
      if (best != 0 && val > stay) {       // uniform: every thread holds the same decision
        const int h = 2047 - (int)(best & 2047u);
#pragma unroll
        for (int u = 0; u < UT_PER; ++u)
          if (tid + u * RF_NT == p) my[u] = h;
        if (tid == 0) {
          slot[p] = h;
          size[gs] -= 1;
          size[h] += 1;
        }
        ++moves;
        gain += (long long)val - (long long)stay;
        moved = true;
      }
      cur ^= 1;
    }
    ++sweeps;
    if constexpr (ROUNDS == RF_MERGE) {    // a node phase ends here: one group sweep, a round
      if (moved && sweeps < max_sweeps) continue;
      if (rounds == 0) node_gain = gain;
      const uint32_t merged =
          rm_group_sweep<LADDER>(wb, tp, nc, nwav, S, slot, size, first, g, t, wkey, my, gain);
      nmerged += merged;
      ++rounds;
      converged = !moved && merged == 0;
      if (merged == 0 || rounds >= max_rounds) break;      // or the sweeps are used up
    } else if constexpr (ROUNDS == RF_SPLIT) {              // ... then the sweeps of `kinds`
      if (moved && sweeps < max_sweeps) continue;
      if (rounds == 0) node_gain = gain;
      uint32_t merged = 0, split = 0;      // kinds is uniform
      if (kinds & HDG_RS_MERGE)
        merged = rm_group_sweep<LADDER>(wb, tp, nc, nwav, S, slot, size, first, g, t, wkey, my,
                                        gain);
      if (kinds & HDG_RS_SPLIT)
        split = rs_split_sweep<LADDER>(wb, tp, nc, slot, size, first, g, t, wkey, my, gain);
      nmerged += merged;
      nsplit += split;
      ++rounds;
      converged = !moved && merged == 0 && split == 0;
      if ((merged == 0 && split == 0) || rounds >= max_rounds) break;
    } else if (!moved) {
      converged = 1;
      break;
    }
  }
  __syncthreads();

  // ---- predicted groups: the final slots, as a forest of smallest members -------------------
  uint32_t* par = reinterpret_cast<uint32_t*>(S[0]);      // the sums are done with
  uint32_t* rnk = reinterpret_cast<uint32_t*>(S[1]);
  for (int i = tid; i < nc; i += RF_NT) first[i] = 0x7FFFFFFF;
  __syncthreads();
  for (int i = tid; i < nc; i += RF_NT) atomicMin(&first[slot[i]], i);
  __syncthreads();
  for (int i = tid; i < nc; i += RF_NT) par[i] = (uint32_t)first[slot[i]];
  __syncthreads();
  const uint32_t G = ut_label(par, rnk, g, wsum, nc);

  const uint32_t TG = ut_true_groups(par, rnk, t, wsum, yb, nc);
  ut_pair_counts(g, t, red, nc);

  // ---- outputs ------------------------------------------------------------------------------
  if (groups)                              // uniform
    for (int i = tid; i < nc; i += RF_NT) groups[i] = (int32_t)g[i];
  __syncthreads();
  if (tid == 0) {
    ut_pair_table(red, G, TG, nc, row);
    u64 nans = 0;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(wb) + (size_t)nc * nc;
    const int tiles = ut_tiles(nc);
    for (int f = 0; f < tiles; ++f) nans += cnt[f];
    row[HDG_RF_MOVES] = moves;
    row[HDG_RF_NAN] = nans;
    qrow[HDG_RF_Q_START] = q_start;
    qrow[HDG_RF_Q_END] = q_start + gain;
    qrow[HDG_RF_Q_SWEEPS] = sweeps;
    qrow[HDG_RF_Q_CONVERGED] = converged;
    if constexpr (ROUNDS != RF_PLAIN) {
      qrow[HDG_RM_Q_ROUNDS] = rounds;
      qrow[HDG_RM_Q_MERGES] = nmerged;
      qrow[HDG_RM_Q_NODE] = q_start + node_gain;
      qrow[HDG_RS_Q_SPLITS] = nsplit;      // 0 without split sweeps
    }
  }
}

__global__ __launch_bounds__(RF_NT) void k_rf_sweep(const int32_t* __restrict__ ws,
                                                    const uint32_t* __restrict__ ybits,
                                                    const int32_t* gin, int32_t* groups,
                                                    u64* __restrict__ ut,
                                                    long long* __restrict__ rq, const int nc,
                                                    const int max_sweeps) {
  const size_t b = blockIdx.x;
  rf_sweep<false, RF_PLAIN>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc),
                         gin ? gin + b * nc : nullptr, nullptr, nullptr, 0.f, groups + b * nc,
                         ut + b * HDG_RF_SLOTS, rq + b * HDG_RF_Q_SLOTS, nc, max_sweeps, 1, 0);
}

// hdg_refine_merge: k_rf_sweep's block with rounds; rq rows of HDG_RM_Q_SLOTS
__global__ __launch_bounds__(RF_NT) void k_rm_sweep(const int32_t* __restrict__ ws,
                                                    const uint32_t* __restrict__ ybits,
                                                    const int32_t* gin, int32_t* groups,
                                                    u64* __restrict__ ut,
                                                    long long* __restrict__ rq, const int nc,
                                                    const int max_sweeps, const int max_rounds) {
  const size_t b = blockIdx.x;
  rf_sweep<false, RF_MERGE>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc),
                        gin ? gin + b * nc : nullptr, nullptr, nullptr, 0.f, groups + b * nc,
                        ut + b * HDG_RF_SLOTS, rq + b * HDG_RM_Q_SLOTS, nc, max_sweeps,
                        max_rounds, HDG_RS_MERGE);
}

// grid (rungs, B): the rungs of a commit are dispatched together and share its matrix in L2;
// outputs [rung][b]
__global__ __launch_bounds__(RF_NT) void k_rl_sweep(const int32_t* __restrict__ ws,
                                                    const uint32_t* __restrict__ ybits,
                                                    const int32_t* __restrict__ merges,
                                                    const float* __restrict__ levels,
                                                    const rl_bounds bounds, int32_t* groups,
                                                    u64* __restrict__ ut,
                                                    long long* __restrict__ rq, const int nc,
                                                    const int max_sweeps) {
  const size_t b = blockIdx.y, o = (size_t)blockIdx.x * gridDim.y + b;
  const size_t n1 = (size_t)nc - 1;
  rf_sweep<true, RF_PLAIN>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc), nullptr,
                        merges ? merges + b * n1 * 2 : nullptr,
                        merges ? levels + b * n1 : nullptr, bounds.tp[blockIdx.x],
                        groups ? groups + o * nc : nullptr, ut + o * HDG_RF_SLOTS,
                        rq + o * HDG_RF_Q_SLOTS, nc, max_sweeps, 1, 0);
}

// hdg_refine_merge_ladder: k_rl_sweep's block with rounds; rq rows of HDG_RM_Q_SLOTS
__global__ __launch_bounds__(RF_NT) void k_rml_sweep(const int32_t* __restrict__ ws,
                                                     const uint32_t* __restrict__ ybits,
                                                     const int32_t* __restrict__ merges,
                                                     const float* __restrict__ levels,
                                                     const rl_bounds bounds, int32_t* groups,
                                                     u64* __restrict__ ut,
                                                     long long* __restrict__ rq, const int nc,
                                                     const int max_sweeps, const int max_rounds) {
  const size_t b = blockIdx.y, o = (size_t)blockIdx.x * gridDim.y + b;
  const size_t n1 = (size_t)nc - 1;
  rf_sweep<true, RF_MERGE>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc), nullptr,
                       merges ? merges + b * n1 * 2 : nullptr,
                       merges ? levels + b * n1 : nullptr, bounds.tp[blockIdx.x],
                       groups ? groups + o * nc : nullptr, ut + o * HDG_RF_SLOTS,
                       rq + o * HDG_RM_Q_SLOTS, nc, max_sweeps, max_rounds,
                       HDG_RS_MERGE);
}

// hdg_refine_split: k_rm_sweep's block, a round's sweeps chosen by `kinds`; rq rows of
// HDG_RS_Q_SLOTS
__global__ __launch_bounds__(RF_NT) void k_rs_sweep(const int32_t* __restrict__ ws,
                                                    const uint32_t* __restrict__ ybits,
                                                    const int32_t* gin, int32_t* groups,
                                                    u64* __restrict__ ut,
                                                    long long* __restrict__ rq, const int nc,
                                                    const int max_sweeps, const int max_rounds,
                                                    const int kinds) {
  const size_t b = blockIdx.x;
  rf_sweep<false, RF_SPLIT>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc),
                            gin ? gin + b * nc : nullptr, nullptr, nullptr, 0.f, groups + b * nc,
                            ut + b * HDG_RF_SLOTS, rq + b * HDG_RS_Q_SLOTS, nc, max_sweeps,
                            max_rounds, kinds);
}

// hdg_refine_split_ladder: k_rml_sweep's block, a round's sweeps chosen by `kinds`
__global__ __launch_bounds__(RF_NT) void k_rsl_sweep(const int32_t* __restrict__ ws,
                                                     const uint32_t* __restrict__ ybits,
                                                     const int32_t* __restrict__ merges,
                                                     const float* __restrict__ levels,
                                                     const rl_bounds bounds, int32_t* groups,
                                                     u64* __restrict__ ut,
                                                     long long* __restrict__ rq, const int nc,
                                                     const int max_sweeps, const int max_rounds,
                                                     const int kinds) {
  const size_t b = blockIdx.y, o = (size_t)blockIdx.x * gridDim.y + b;
  const size_t n1 = (size_t)nc - 1;
  rf_sweep<true, RF_SPLIT>(ws + b * rf_commit_words(nc), ut_label_rows(ybits, (int)b, nc),
                           nullptr, merges ? merges + b * n1 * 2 : nullptr,
                           merges ? levels + b * n1 : nullptr, bounds.tp[blockIdx.x],
                           groups ? groups + o * nc : nullptr, ut + o * HDG_RF_SLOTS,
                           rq + o * HDG_RS_Q_SLOTS, nc, max_sweeps, max_rounds, kinds);
}

// what the six entry points check first, in this order.  max_rounds: NULL for the calls
// without rounds; kinds: NULL for the calls that are not hdg_refine_split's
inline int rf_check_call(const hdg_shape* s, const int32_t rule, const int32_t max_sweeps,
                         const int32_t* max_rounds, const int32_t* kinds, const int32_t flags,
                         const char* who) {
  if (const int rc = ut_check_shape(s, who)) return rc;
  if (const int rc = ut_check_rule(rule, who)) return rc;
  if (max_sweeps < 1 || max_sweeps > HDG_RF_MAX_SWEEPS)
    return fail(HDG_EINVAL, "%s: max_sweeps must be in [1, %d] (got %d)", who, HDG_RF_MAX_SWEEPS,
                (int)max_sweeps);
  if (max_rounds && (*max_rounds < 1 || *max_rounds > HDG_RM_MAX_ROUNDS))
    return fail(HDG_EINVAL, "%s: max_rounds must be in [1, %d] (got %d)", who, HDG_RM_MAX_ROUNDS,
                (int)*max_rounds);
  if (kinds && (*kinds < 1 || *kinds > (HDG_RS_MERGE | HDG_RS_SPLIT)))
    return fail(HDG_EINVAL, "%s: kinds must be HDG_RS_MERGE, HDG_RS_SPLIT or both (got %d)", who,
                (int)*kinds);
  if (flags != 0) return fail(HDG_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)flags);
  return 0;
}

// hdg_refine (max_rounds NULL), hdg_refine_merge (kinds NULL) and hdg_refine_split under the
// name `who`: the checks, the weights launch, the sweep launch
int rf_call(const char* who, const hdg_shape* s, const hdg_batch* bt, const float* probs,
            const float threshold, const int32_t rule, const int32_t max_sweeps,
            const int32_t* max_rounds, const int32_t* kinds, const int32_t flags,
            const int32_t* groups_in,
            int32_t* groups, uint64_t* ut, int64_t* rq, void* workspace, void* stream) {
  if (const int rc = rf_check_call(s, rule, max_sweeps, max_rounds, kinds, flags, who)) return rc;
  const float tp = ut_link_bound(rule, threshold);
  if (!std::isfinite(threshold) || !std::isfinite(tp))
    return fail(HDG_EINVAL, "%s: threshold %g gives no finite link bound", who,
                (double)threshold);
  if (!bt || !bt->ybits || !probs || !groups || !ut || !rq || !workspace)
    return fail(HDG_EINVAL, "%s: NULL pointer (batch, batch->ybits, probs, groups, ut, "
                            "rq or workspace)", who);
  if (const int rc = ut_check_workspace(workspace, who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nc = s->nc;
  hipLaunchKernelGGL(k_rf_weights, dim3((unsigned)ut_tiles(nc), (unsigned)s->batch),
                     dim3(UT_LINK_NT), 0, st, probs, (int32_t*)workspace, nc, (int)rule, tp);
  if (const int rc = ut_launched(who, "weights")) return rc;
  if (kinds)
    hipLaunchKernelGGL(k_rs_sweep, dim3((unsigned)s->batch), dim3(RF_NT), 0, st,
                       (const int32_t*)workspace, bt->ybits, groups_in, groups, (u64*)ut,
                       (long long*)rq, nc, (int)max_sweeps, (int)*max_rounds, (int)*kinds);
  else if (max_rounds)
    hipLaunchKernelGGL(k_rm_sweep, dim3((unsigned)s->batch), dim3(RF_NT), 0, st,
                       (const int32_t*)workspace, bt->ybits, groups_in, groups, (u64*)ut,
                       (long long*)rq, nc, (int)max_sweeps, (int)*max_rounds);
  else
    hipLaunchKernelGGL(k_rf_sweep, dim3((unsigned)s->batch), dim3(RF_NT), 0, st,
                       (const int32_t*)workspace, bt->ybits, groups_in, groups, (u64*)ut,
                       (long long*)rq, nc, (int)max_sweeps);
  return ut_launched(who, "sweep");
}

// hdg_refine_ladder (max_rounds NULL), hdg_refine_merge_ladder (kinds NULL) and
// hdg_refine_split_ladder under the name `who`
int rl_call(const char* who, const hdg_shape* s, const hdg_batch* bt, const float* probs,
            const float* thresholds, const int32_t n_rungs, const int32_t rule,
            const int32_t max_sweeps, const int32_t* max_rounds, const int32_t* kinds,
            const int32_t flags, const int32_t* merges, const float* levels, int32_t* groups, uint64_t* ut,
            int64_t* rq, void* workspace, void* stream) {
  if (const int rc = rf_check_call(s, rule, max_sweeps, max_rounds, kinds, flags, who)) return rc;
  if (n_rungs < 1 || n_rungs > HDG_RL_MAX_RUNGS)
    return fail(HDG_EINVAL, "%s: n_rungs must be in [1, %d] (got %d)", who, HDG_RL_MAX_RUNGS,
                (int)n_rungs);
  if (!thresholds) return fail(HDG_EINVAL, "%s: NULL pointer (thresholds)", who);
  rl_bounds bounds = {};
  for (int k = 0; k < n_rungs; ++k) {      // each rung's t' once, here, as hdg_refine forms it
    bounds.tp[k] = ut_link_bound(rule, thresholds[k]);
    if (!std::isfinite(thresholds[k]) || !std::isfinite(bounds.tp[k]))
      return fail(HDG_EINVAL, "%s: rung %d: threshold %g gives no finite link bound", who, k,
                  (double)thresholds[k]);
  }
  if ((merges == nullptr) != (levels == nullptr))
    return fail(HDG_EINVAL, "%s: merges and levels come together or not at all", who);
  if (!bt || !bt->ybits || !probs || !ut || !rq || !workspace)
    return fail(HDG_EINVAL, "%s: NULL pointer (batch, batch->ybits, probs, ut, rq or workspace)",
                who);
  if (const int rc = ut_check_workspace(workspace, who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nc = s->nc;
  hipLaunchKernelGGL(k_rl_weights, dim3((unsigned)ut_tiles(nc), (unsigned)s->batch),
                     dim3(UT_LINK_NT), 0, st, probs, (int32_t*)workspace, nc, (int)rule);
  if (const int rc = ut_launched(who, "weights")) return rc;
  const dim3 grid((unsigned)n_rungs, (unsigned)s->batch);
  if (kinds)
    hipLaunchKernelGGL(k_rsl_sweep, grid, dim3(RF_NT), 0, st, (const int32_t*)workspace,
                       bt->ybits, merges, levels, bounds, groups, (u64*)ut, (long long*)rq, nc,
                       (int)max_sweeps, (int)*max_rounds, (int)*kinds);
  else if (max_rounds)
    hipLaunchKernelGGL(k_rml_sweep, grid, dim3(RF_NT), 0, st, (const int32_t*)workspace,
                       bt->ybits, merges, levels, bounds, groups, (u64*)ut, (long long*)rq, nc,
                       (int)max_sweeps, (int)*max_rounds);
  else
    hipLaunchKernelGGL(k_rl_sweep, grid, dim3(RF_NT), 0, st, (const int32_t*)workspace,
                       bt->ybits, merges, levels, bounds, groups, (u64*)ut, (long long*)rq, nc,
                       (int)max_sweeps);
  return ut_launched(who, "sweep");
}

}  // namespace

extern "C" size_t hdg_refine_workspace_bytes(const hdg_shape* s, int32_t flags) {
  if (ut_check_shape(s, "hdg_refine_workspace_bytes")) return 0;
  (void)flags;                             // no flag is defined; hdg_refine rejects any bit
  return (size_t)s->batch * rf_commit_words(s->nc) * sizeof(int32_t);
}

extern "C" int hdg_refine(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                          float threshold, int32_t rule, int32_t max_sweeps, int32_t flags,
                          const int32_t* groups_in, int32_t* groups, uint64_t* ut, int64_t* rq,
                          void* workspace, void* stream) {
  return rf_call("hdg_refine", s, bt, probs, threshold, rule, max_sweeps, nullptr, nullptr,
                 flags, groups_in, groups, ut, rq, workspace, stream);
}

extern "C" int hdg_refine_merge(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                                float threshold, int32_t rule, int32_t max_sweeps,
                                int32_t max_rounds, int32_t flags, const int32_t* groups_in,
                                int32_t* groups, uint64_t* ut, int64_t* rq, void* workspace,
                                void* stream) {
  return rf_call("hdg_refine_merge", s, bt, probs, threshold, rule, max_sweeps, &max_rounds,
                 nullptr, flags, groups_in, groups, ut, rq, workspace, stream);
}

extern "C" size_t hdg_refine_ladder_workspace_bytes(const hdg_shape* s, int32_t flags) {
  if (ut_check_shape(s, "hdg_refine_ladder_workspace_bytes")) return 0;
  (void)flags;                             // no flag is defined; hdg_refine_ladder rejects any bit
  return (size_t)s->batch * rf_commit_words(s->nc) * sizeof(int32_t);     // no factor n_rungs
}

extern "C" int hdg_refine_ladder(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                                 const float* thresholds, int32_t n_rungs, int32_t rule,
                                 int32_t max_sweeps, int32_t flags, const int32_t* merges,
                                 const float* levels, int32_t* groups, uint64_t* ut, int64_t* rq,
                                 void* workspace, void* stream) {
  return rl_call("hdg_refine_ladder", s, bt, probs, thresholds, n_rungs, rule, max_sweeps,
                 nullptr, nullptr, flags, merges, levels, groups, ut, rq, workspace, stream);
}

extern "C" int hdg_refine_merge_ladder(const hdg_shape* s, const hdg_batch* bt,
                                       const float* probs, const float* thresholds,
                                       int32_t n_rungs, int32_t rule, int32_t max_sweeps,
                                       int32_t max_rounds, int32_t flags, const int32_t* merges,
                                       const float* levels, int32_t* groups, uint64_t* ut,
                                       int64_t* rq, void* workspace, void* stream) {
  return rl_call("hdg_refine_merge_ladder", s, bt, probs, thresholds, n_rungs, rule, max_sweeps,
                 &max_rounds, nullptr, flags, merges, levels, groups, ut, rq, workspace, stream);
}

extern "C" int hdg_refine_split(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                                float threshold, int32_t rule, int32_t max_sweeps,
                                int32_t max_rounds, int32_t kinds, int32_t flags,
                                const int32_t* groups_in, int32_t* groups, uint64_t* ut,
                                int64_t* rq, void* workspace, void* stream) {
  return rf_call("hdg_refine_split", s, bt, probs, threshold, rule, max_sweeps, &max_rounds,
                 &kinds, flags, groups_in, groups, ut, rq, workspace, stream);
}

extern "C" int hdg_refine_split_ladder(const hdg_shape* s, const hdg_batch* bt,
                                       const float* probs, const float* thresholds,
                                       int32_t n_rungs, int32_t rule, int32_t max_sweeps,
                                       int32_t max_rounds, int32_t kinds, int32_t flags,
                                       const int32_t* merges, const float* levels,
                                       int32_t* groups, uint64_t* ut, int64_t* rq,
                                       void* workspace, void* stream) {
  return rl_call("hdg_refine_split_ladder", s, bt, probs, thresholds, n_rungs, rule, max_sweeps,
                 &max_rounds, &kinds, flags, merges, levels, groups, ut, rq, workspace, stream);
}
