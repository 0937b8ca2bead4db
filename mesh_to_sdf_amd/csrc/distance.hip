// distance.hip — nearest-triangle distance + sign resolve: the walks, the dominant kernels (gfx950), and their policy.
//
// Semantics: D(p) = min over ALL triangles of geo.rs:26-30 in the reference's
// f32 operation order; sign by the rule the caller's SignMethod / AccelerationMethod selects.
//
//   k_packet : one wave = 64 spatially adjacent points (a 4x4x4 brick of voxels, or 64 Morton-
//              sorted queries).  The wave walks the stackless pre-order BVH TOGETHER: the node
//              index is wave-uniform (SGPR), node and triangle records arrive through scalar
//              loads, each lane tests its own point, and a subtree is skipped when the ballot of
//              "my bound reaches this box" is empty.  No per-lane stack, no divergence, no gather.
//   k_lane   : one point per lane, every lane on its own through the tree (k_lane_q: sorted queries).
//
// Pruning is conservative: a subtree is dropped only if its box is farther than the lane's
// current best by a margin that covers f32 rounding of both the box test and the reference
// arithmetic (see prune_bound), so the minimum is the brute-force minimum bit for bit.
//
// This unit also decides which path a call takes (choose_grid_walk) and strings the stages together (prepare_grid_walk,
// launch_grid_walk, launch_query_walk).  The other stages are units of their own: seeds.hip (seed lattices), cut.hip (k_cut),
// brute.hip (all pairs, same arithmetic: k_brute and the tiny paths), query_order.hip (Morton order and packets of generic
// queries), peer_push.hip (copies to peer devices); dist.hip.h holds what they share.
#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "geo.hip.h"
#include "tuning.h"
#include "walk.hip.h"
#include "dist.hip.h"

namespace m2s {

namespace {

template <int AXIS>
__device__ __forceinline__ uint32_t stab_count(const DeviceMesh& mesh, f3 p) {
  uint32_t count = 0;
  uint32_t node = 0;
  while (node < mesh.n_nodes) {
    node = __builtin_amdgcn_readfirstlane(node);
    const NodeRec nr = record_at(mesh.nodes, node);
    const bool hit = ray_meets_box<AXIS>(p, mk3(nr.mnx, nr.mny, nr.mnz), mk3(nr.mxx, nr.mxy, nr.mxz));
    if (__ballot(hit) == 0ull) { node = nr.skip; continue; }
    if (nr.tri >= 0) {
      const uint32_t cnt = (nr.skip - node + 1u) >> 1;
      for (uint32_t k = 0; k < cnt; ++k) {
        uint32_t vi;                                   // (a wave-uniform index through a VGPR: a broadcast out of the vector L1, as record_at_vec)
        asm("v_mov_b32_e32 %0, %1" : "=v"(vi) : "s"(3u * ((uint32_t)nr.tri + k)));
        const float4 c0 = mesh.corners[vi], c1 = mesh.corners[vi + 1u], c2 = mesh.corners[vi + 2u];
        const f3 a = mk3(c0.x, c0.y, c0.z), b = mk3(c0.w, c1.x, c1.y), c = mk3(c1.z, c1.w, c2.x);
        f3 mn, mx;
        triangle_bounding_box(a, b, c, &mn, &mx);     // the candidate rule is per triangle: ITS padded box
        float t;
        const bool h = ray_meets_box<AXIS>(p, mn, mx) & ray_triangle_aligned<AXIS>(p, a, b, c, &t);
        count += h ? 1u : 0u;
      }
      node = nr.skip;
    } else {
      node = node + 1;
    }
  }
  return count;
}

// The same count with the ray-triangle tests run densely (cf. DeferQueue below): the packet's 64 sorted queries are neighbours, not
// a brick — a leaf triangle's padded box is met by a few lanes' rays, and its test (box, 18 + ~40 instructions) ran wave-wide for
// them.  Here a leaf queues (lane, triangle) for the lanes whose ray meets the leaf's box, 64 pairs are tested at a time (each lane
// one pair: the owner's point by lane permutes, the corners by a gather), and a hit bumps the owner's LDS counter.  Same candidates
// per lane (a lane whose ray misses the leaf's box cannot meet a triangle's box inside it), same test: the same count.
// `lds`: 192 words of this wave's.
template <int AXIS>
__device__ __forceinline__ uint32_t stab_count_dense(const DeviceMesh& mesh, f3 p, uint32_t* lds) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* q = lds;
  uint32_t* hits = lds + 128;
  uint32_t head = 0, n = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  hits[lane] = 0u;
  auto flush = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t take = min(n, 64u);
    const bool valid = lane < take;
    const uint32_t e = valid ? q[(head + lane) & 127u] : 0u;
    const uint32_t v = e & 63u, vi = 3u * (e >> 6);
    const f3 pv = mk3(__shfl(p.x, (int)v), __shfl(p.y, (int)v), __shfl(p.z, (int)v));
    const float4 c0 = mesh.corners[vi], c1 = mesh.corners[vi + 1u], c2 = mesh.corners[vi + 2u];
    const f3 a = mk3(c0.x, c0.y, c0.z), b = mk3(c0.w, c1.x, c1.y), c = mk3(c1.z, c1.w, c2.x);
    f3 mn, mx;
    triangle_bounding_box(a, b, c, &mn, &mx);     // the candidate rule is per triangle: ITS padded box
    float t;
    const bool h = ray_meets_box<AXIS>(pv, mn, mx) & ray_triangle_aligned<AXIS>(pv, a, b, c, &t);
    if (valid & h) atomicAdd(&hits[v], 1u);
    head = (head + take) & 127u;
    n -= take;
  };
  uint32_t node = 0;
  while (node < mesh.n_nodes) {
    node = __builtin_amdgcn_readfirstlane(node);
    const NodeRec nr = record_at(mesh.nodes, node);
    const bool hit = ray_meets_box<AXIS>(p, mk3(nr.mnx, nr.mny, nr.mnz), mk3(nr.mxx, nr.mxy, nr.mxz));
    const unsigned long long hb = __ballot(hit);
    if (hb == 0ull) { node = nr.skip; continue; }
    if (nr.tri >= 0) {
      const uint32_t cnt = (nr.skip - node + 1u) >> 1;
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(hb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hb, 0u));
      for (uint32_t k = 0; k < cnt; ++k) {
        if (hit) q[(head + n + rank) & 127u] = lane | (((uint32_t)nr.tri + k) << 6);
        n += (uint32_t)__popcll(hb);
        if (n >= 64u) flush();
      }
      node = nr.skip;
    } else {
      node = node + 1;
    }
  }
  while (n != 0u) flush();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return hits[lane];
}

// ---- the packet walk ------------------------------------------------------------------------
// Wave-uniform counters of one packet's walk (SGPRs; only the M2S_STATS variant keeps them).
struct WalkStats {
  uint32_t box = 0, ext = 0, leaf = 0, pruned = 0, slab = 0, sphere = 0, pairs = 0;
  uint32_t node_lanes = 0, pre_lanes = 0;   // lanes whose bound reaches the node / that take part in a leaf's pre-test by that measure
  // the packet's seed triangle as the walk meets it again (walk_span SEEDED): its slot — set by k_packet whether or not the walk passes over
  // it —, how often the walk met it, the lanes whose bound reached its leaf then (the (lane, seed) pairs the DEFER 3 walk would queue) and,
  // where it was not passed over, how many of those passed the pre-test (and were evaluated a second time)
  uint32_t seed = 0xffffffffu, seed_met = 0, seed_lanes = 0, seed_passed = 0;
  bool seed_inside = false;   // on the way down inside the seed's collapsed leaf
};

// ---- split walk -------------------------------------------------------------------------------
// When the dispatcher has handed out the last packet of a launch, the wave slots fall idle one by one while the packets still
// running — the heavy ones: blob-1M's heaviest packet does 4 004 node tests + 2 220 exact evaluations and is 3.4 ms alone on a
// SIMD — decide when the launch ends.  So a walk may be SUSPENDED: from then on it keeps walking the TOP of what is left (the node
// tests there prune most of it), but a subtree of at most `emit_max` bytes of records that survives its test is not entered: it
// becomes an ITEM of a follow-up launch in which any wave may take it, starting from the bests the packet ends with (the seed is
// within 10 % of a perfect bound, so an item loses little by not seeing what the others find).  The items' minima are merged
// with atomic minima on per-voxel words (non-negative floats order like their bit patterns; min is associative and commutative:
// the same bits as one walk), and k_split_finish turns the merged minima into signed distances.  (A first form cut the unwalked
// record RANGES into eight equal pieces: a piece that starts in the middle of a subtree has lost its ancestors' pruning, seven of
// eight pieces lie where one test of an ancestor would have dropped them, and the follow-up rounds of 128^3 x blob-100k took longer
// than the walk — 46 000 items, 1.7 ms.)
//
// WHEN to suspend needs no model of the work: the launch measures itself.  The first workgroup an XCD is handed stamps the time
// (s_memrealtime, 100 MHz) into that XCD's start word, the last one into its flag ("the dispatcher has run dry here": from now on
// wave slots of this XCD fall idle).  The time between the two, divided by the rounds of the chip's wave slots that the launch is deep
// (host: packets / slots - 1, at least 1), is how long an ordinary packet of THIS launch takes at full occupancy; a walk that has done
// `grace` work units looks every CHECK_EVERY units, and once the flag has been up for `patience` such packet times it is suspended:
// every ordinary packet that was running when the flag went up has finished by then, what is left are the stragglers.  The
// follow-up rounds work through their items with a fixed set of waves striding the list; the first wave of an XCD to run out raises
// the round's flag, and an item still being walked `grace` units later is suspended in its turn (items are bounded — at most emit_max
// records — so a work count serves there).  The last round walks to the end.  (Forms that did not work: suspending everything still
// running when the flag goes up — at 128^3, four rounds deep, that is a quarter of all packets, ordinary ones, and the rounds did more
// work than the walk had left; a fixed number of work units after the flag — right for one grid, 40 % slower on the next: 96^3 wants
// 1024, 128^3 512, a 1 M-triangle slab 256; counting running packets with two atomics per packet on a per-XCD word — 45 ns each,
// serialised: 1.2 -> 7 ms.)
// Work is counted where it is done, at the leaves — 3 units per leaf visited (the node tests that led to it), 1 per
// pre-test, 4 per exact evaluation (25 : 20 : 140 vector instructions) — so the inner nodes' path carries no bookkeeping at all.
// The words are per XCD because a word everybody reads at device scope is a serial resource (one flag, one agent-scope load per
// packet: + 10 ms on the 512^3 walk — 2 M loads, ~5 ns each at the memory side).  Workgroup b of a one-dimensional launch runs on
// XCD b % 8; writer and readers share that XCD's L2, so the stores are the plain kind (the line stays in that L2) and the loads
// only have to pass the CU's own L1, which other CUs' stores never refresh: non-temporal loads (L2-served; a workgroup-scope `sc0`
// load hits the L1 like a plain one and kept seeing the flag down).  A stale word (or another dispatch order) would cost time,
// never a result.  All of it is inline asm: to the compiler these are not memory operations, so nothing around them is reordered
// or demoted for their sake (a store at the top of k_packet moved every wave-uniform load of its prologue — seed index, mesh scale —
// from the scalar to the vector unit, "may be clobbered", behind the cut list's cold miss: + 20 %).  Every string starts with
// s_nop 4: the compiler does not see into it, and an address that has just come out of a spill lane (a VALU write of an SGPR) needs
// five wait states before a memory instruction may read it — without them a follow-up round loaded its flag from garbage addresses.
// The SplitCtl of a launch that does not split: no counters (split_arm arms nothing, and only the split forms call it), and the plain forms' one
// launch word under its own name (common.h SplitCtl::plain_seed_none, the bytes of `grace`, which a plain form must never read as such).
static_assert(offsetof(SplitCtl, plain_seed_none) == offsetof(SplitCtl, grace) && sizeof(SplitCtl) == 64, "the word shares grace's bytes: the split forms' argument list is unchanged");
inline SplitCtl plain_ctl(uint32_t seed_none) { SplitCtl ctl{}; ctl.plain_seed_none = seed_none; return ctl; }
constexpr uint32_t SPLIT_CHECK_EVERY = 64;
constexpr uint32_t SPLIT_CONTINUATION = 0x80000000u;   // item tag (with the slot): a suspended packet, not a subtree
struct SplitState {
  uint32_t units = 0, next_check = 0xffffffffu;   // work done so far; next look at the flag (never, unless armed)
  const uint32_t* flag_addr = nullptr;            // this XCD's flag of the launch (k_packet: the time it went up, odd; rounds: 1)
  uint32_t patience_q8 = 0;                       // k_packet: patience / rounds-before-the-flag, in 1/256
  uint32_t grace = 0;
  bool suspended = false, flag_seen = false;
  uint32_t resume_end = 0;                        // suspended: the end of the range that was being walked
  uint32_t* n_ranges = nullptr;                   // k_packet: the caller's count of ranges (zeroed on suspension: its loop ends too)
};
__device__ __forceinline__ uint32_t* split_flag_addr(const SplitCtl& ctl, uint32_t round) {   // this XCD's flag of the round
  return ctl.cnt + 16u + round * 16u + (blockIdx.x & 7u);
}
__device__ __forceinline__ uint32_t split_peek(const uint32_t* addr) {          // wave-uniform address, wave-uniform result
  uint32_t v;
  const uint32_t zero = 0;
  asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2 nt\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(zero), "s"(addr));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ void split_poke(uint32_t* addr, uint32_t value) {   // call with one lane active
  const uint32_t zero = 0;
  asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2" : : "v"(zero), "v"(value), "s"(addr));
}
__device__ __forceinline__ uint32_t split_now() { return (uint32_t)__builtin_amdgcn_s_memrealtime(); }   // 10 ns ticks; differences survive the wrap
__device__ __forceinline__ void split_arm(SplitState& sp, const SplitCtl& ctl, uint32_t round, bool may_suspend) {
  if (ctl.cnt == nullptr || !may_suspend) return;
  sp.flag_addr = split_flag_addr(ctl, round);
  sp.next_check = ctl.grace;
  sp.grace = ctl.grace;
  sp.patience_q8 = ctl.patience_q8;
}
// k_packet: has this XCD's flag been up for `patience` ordinary packet times?  (the start word lies 8 words behind the flag)
__device__ __forceinline__ bool split_stragglers_only(const SplitState& sp) {
  const uint32_t up = split_peek(sp.flag_addr);
  if (up == 0u) return false;
  const uint32_t start = split_peek(sp.flag_addr + 8), now = split_now();
  const uint32_t fill = up - start;                                       // time it took to hand out this XCD's packets
  const uint32_t allowed = (uint32_t)(((unsigned long long)fill * sp.patience_q8) >> 8);
  return now - up >= allowed;
}

// A suspended PACKET (k_packet) leaves its bests and ONE item — "go on at record `off` of range `range`" — and gives up its wave slot;
// a wave of round 1 walks the top of what is left and turns the subtrees that survive into the items of round 2 (k_split_round).
// false: no accumulator slot or list entry left (the packet then walks on by itself).
template <int MODE>
__device__ __forceinline__ bool split_handover(const SplitCtl& split, uint32_t packet, uint32_t range, uint32_t off, const Best<MODE>& best, int* err) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t slot = 0, idx = 0;
  if (lane == 0u) slot = atomicAdd(&split.cnt[0], 1u);
  slot = __builtin_amdgcn_readfirstlane(slot);
  if (slot >= split.cap_slots) return false;
  if (lane == 0u) idx = atomicAdd(&split.cnt[2], 1u);
  idx = __builtin_amdgcn_readfirstlane(idx);
  if (idx >= split.cap_items) {
    if (lane == 0u) split.slot_packet[slot] = 0xffffffffu;                  // the slot stays empty
    return false;
  }
  constexpr uint32_t AW = MODE == MODE_NORMAL_FOLD ? 128u : 64u;
  uint32_t* acc = split.acc + (size_t)slot * AW;
  acc[lane] = __float_as_uint(best.d2);
  if (MODE == MODE_NORMAL_FOLD) {
    acc[64 + lane] = __float_as_uint(best.d2pos);
    if (best.nan) atomicOr(err, ERRF_NAN);
  }
  if (lane == 0u) {
    split.items[idx] = make_uint4(packet, off, range, slot | SPLIT_CONTINUATION);
    split.slot_packet[slot] = packet;
  }
  return true;
}

// Where a suspended walk leaves the subtrees it does not enter: slots of the next round's list, reserved 64 at a time.
struct EmitState {
  uint4* list = nullptr;
  uint32_t* count = nullptr;          // the list's fill counter
  uint32_t cap = 0;
  uint32_t base = 0, used = 0, room = 0;
  uint32_t min_bytes = 0xffffffffu, max_bytes = 0;   // subtrees of min_bytes .. max_bytes of records are handed over; min = ~0: nothing is
  uint32_t packet = 0, slot = 0;
};
__device__ __forceinline__ void emit_begin(EmitState& em, const SplitCtl& ctl, uint32_t next_round, uint32_t packet, uint32_t slot) {
  em.list = ctl.items + (size_t)(next_round - 1u) * ctl.cap_items;
  em.count = ctl.cnt + 1u + next_round;
  em.cap = ctl.cap_items;
  em.min_bytes = ctl.emit_min;
  em.max_bytes = ctl.emit_max;
  em.packet = packet;
  em.slot = slot;
}
// The unused part of the reserved block becomes empty items (first == end): the list has no holes of stale data.
__device__ __forceinline__ void emit_close(EmitState& em) {
  const uint32_t i = em.base + em.used + (threadIdx.x & 63u);
  if (i < em.base + em.room && i < em.cap) em.list[i] = make_uint4(em.packet, 0u, 0u, em.slot);
  em.used = em.room;
}
// One more block of 64 slots; when the list is full, emission is switched off (the walk then enters everything itself).
__device__ __forceinline__ void emit_reserve(EmitState& em) {
  uint32_t base = 0;
  if ((threadIdx.x & 63u) == 0u) base = atomicAdd(em.count, 64u);
  em.base = __builtin_amdgcn_readfirstlane(base);
  em.used = 0;
  em.room = 64u;
  if (em.base + 64u > em.cap) {       // (what lies below the cap is this wave's to blank)
    emit_close(em);
    em.room = 0;
    em.min_bytes = 0xffffffffu;
  }
}

// ---- dense exact evaluations (DEFER) ----------------------------------------------------------
// Where a brick meets many triangles (a grid coarse against the mesh: 128^3 x blob-100k) an exact evaluation serves 7 - 18 of the
// wave's 64 lanes — the others' pre-test bound does not reach the triangle — and costs the wave its ~140 instructions all the same.
// Here the leaf only QUEUES (voxel lane, triangle) pairs for the lanes that are reached (one LDS word per pair, written at the lane's
// rank in the ballot), and whenever 64 pairs have come together every lane evaluates ONE of them: it fetches that voxel's point with
// three lane permutes and the pair's triangle record with a gather (pairs of one triangle sit in neighbouring lanes: the same cache
// line), and folds the result into the voxel's slot with an LDS minimum on the f32 bits (non-negative floats order like their
// bits; a NaN's bits lie above +inf's and never win, as fminf never takes it).  The lanes' bounds are refreshed from the slots after
// every batch: they lag by at most one batch, which costs pairs (cheap: a 64th of an evaluation each), never a result — the set of
// triangles evaluated for a voxel only grows, the minimum of the same arithmetic is the same bits.
// The slots hold what Best<MODE> holds: d2 bits; Normal fold: + d2pos bits and a NaN flag; nearest-with-normal: the 64-bit key
// (d2 bits, triangle index, !positive) whose minimum is the lexicographic rule of rtree.rs:118-123 (as the lane walk's LaneShare).
template <int MODE>
struct DeferLayout {
  static constexpr uint32_t SLOT_WORDS = MODE == MODE_NORMAL_FOLD ? 192u : MODE == MODE_NEAREST_NORMAL ? 128u : 64u;
  static constexpr uint32_t DWORDS = (256u + SLOT_WORDS) / 2u;     // the LDS block of one wave, in 8-byte words: two rings + the slots
};
// DEFER = 2: a triangle that DEFER_DIRECT_LANES or more lanes reach is evaluated wave-wide at once, as without the queue.  For grids
// much finer than the mesh — 1024^3 over a flat 100 k-triangle sheet, 0.006 triangles per brick: far from the surface ONE triangle
// is the nearest for most of a brick, 47 of 64 lanes per evaluation — the queue has nothing to compact (walk, direct / queued /
// both: sheet-100k 1024^3 69.0 / 71.9 / 65.4 ms, blob-100k 1024^3 35.6 / 34.0 / 33.6).  Its own variant, because the second
// evaluation body costs the dense regime 3 - 6 % by being there (128^3 x blob-100k 1.02 -> 1.09 ms, 256^3 1.74 -> 1.80).
constexpr uint32_t DEFER_DIRECT_LANES = 48;
struct DeferQueue {
  uint32_t* q;          // LDS: 128 pair words (ring), lane | triangle slot << 6: pairs that passed the pre-test
  uint32_t* slot;       // LDS: the running results of the 64 voxels (DeferLayout)
  uint32_t head, n;     // wave-uniform
  uint32_t* q1;         // LDS: 128 pair words (ring): pairs whose lane's bound reaches the LEAF, waiting for the pre-test (DEFER = 3)
  uint32_t head1, n1;
};
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The owner lane's value of a queued pair: ds_bpermute takes the source lane as a byte address (lane << 2), formed ONCE per batch by
// owner_addr and shared by the batch's three or four fetches.  (__shfl forms it as ((self & 64) | lane) << 2: the compiler cannot see that a
// wave has no lane >= 64, and `self & 64` cost the walk a VGPR for its whole length.)  Pair words keep the lane in bits 0..5.
__device__ __forceinline__ uint32_t owner_addr(uint32_t pair) { return (pair & 63u) << 2; }
__device__ __forceinline__ float owner_fetch(uint32_t addr, float x) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute((int)addr, __float_as_int(x)));
}
template <int MODE>
__device__ __forceinline__ unsigned long long defer_key(const Best<MODE>& x) {
  return ((unsigned long long)__float_as_uint(x.d2) << 32) | ((unsigned long long)(x.idx & 0x7fffffffu) << 1) | (x.pos ? 0ull : 1ull);
}
template <int MODE>
__device__ __forceinline__ DeferQueue defer_begin(unsigned long long* lds) {
  const uint32_t lane = threadIdx.x & 63u;
  DeferQueue dq = {reinterpret_cast<uint32_t*>(lds), reinterpret_cast<uint32_t*>(lds) + 256, 0u, 0u, reinterpret_cast<uint32_t*>(lds) + 128, 0u, 0u};
  if (MODE == MODE_NEAREST_NORMAL) reinterpret_cast<unsigned long long*>(dq.slot)[lane] = 0x7f800000ffffffffull;   // (+inf, none)
  else {
    dq.slot[lane] = 0x7f800000u;
    if (MODE == MODE_NORMAL_FOLD) { dq.slot[64u + lane] = 0x7f800000u; dq.slot[128u + lane] = 0u; }
  }
  return dq;
}
// What the unsigned evaluation of a queued pair reads of its triangle: bytes [0, 48) of the TriRec, the three vertices and the class.  Every
// lane has its own triangle here, so each 16-byte row of the record is a 64-lane gather; the stored edge rows, which the wave-wide forms get
// as scalar operands for nothing, would be three more of them, and the compiler used to sink two of the six into the regions that use them,
// each behind a wait of its own: up to three L2 round trips in a row per batch.  pair_verts_request issues the three loads together, ordinary
// cached loads; pair_verts_arrive, placed behind the owner fetches, is an empty statement that takes the ten words as operands: no load can
// be moved past it, and the one wait in front of it covers the batch.  The edges are formed on the VALU (geo.hip.h point_triangle_pair_dist2).
// The Normal fold and nearest-with-normal need the edge rows' fourth components (the raw normal) and keep gathering the whole record.
struct PairVerts {
  f3 a, b, c;
  uint32_t cls;
};
__device__ __forceinline__ PairVerts pair_verts_request(const TriRec* tris, uint32_t t) {
  static_assert(offsetof(TriRec, cls) == 12 && offsetof(TriRec, bx) == 16 && offsetof(TriRec, cx) == 32, "a | cls, b, c in the first three rows");
  const TriRec& r = tris[t];   // a | cls as one dwordx4, b and c as dwordx3: no register for the words nobody reads
  return {mk3(r.ax, r.ay, r.az), mk3(r.bx, r.by, r.bz), mk3(r.cx, r.cy, r.cz), r.cls};
}
__device__ __forceinline__ void pair_verts_arrive(PairVerts& pr) {
  asm volatile("" : "+v"(pr.a.x), "+v"(pr.a.y), "+v"(pr.a.z), "+v"(pr.cls), "+v"(pr.b.x), "+v"(pr.b.y), "+v"(pr.b.z), "+v"(pr.c.x), "+v"(pr.c.y), "+v"(pr.c.z));
}
// Evaluates up to 64 queued pairs (all of them when fewer are left) and refreshes the lanes' results from their slots.
template <int MODE>
__device__ __forceinline__ void defer_flush(const DeviceMesh& mesh, f3 p, DeferQueue& dq, Best<MODE>& best) {
  const uint32_t lane = threadIdx.x & 63u;
  wave_lds_sync();
  const uint32_t take = min(dq.n, 64u);
  const bool valid = lane < take;
  const uint32_t e = valid ? dq.q[(dq.head + lane) & 127u] : 0u;
  const uint32_t v = e & 63u, t = e >> 6, va = owner_addr(e);
  PairVerts pr = {};
  if (MODE == MODE_UNSIGNED) pr = pair_verts_request(mesh.tris, t);
  const f3 pv = mk3(owner_fetch(va, p.x), owner_fetch(va, p.y), owner_fetch(va, p.z));
  if (MODE == MODE_UNSIGNED) pair_verts_arrive(pr);
  Best<MODE> one;
  // (a NaN d2 goes to the LDS minimum as it is: its bits lie above +inf's, with either sign, and never win — what fminf made of it before)
  if (MODE == MODE_UNSIGNED) one.d2 = point_triangle_pair_dist2(pv, pr.a, pr.b, pr.c, pr.cls);
  else eval_triangle<MODE>(one, pv, mesh.tris[t]);
  if (valid) {
    if (MODE == MODE_NEAREST_NORMAL) atomicMin(&reinterpret_cast<unsigned long long*>(dq.slot)[v], defer_key<MODE>(one));
    else {
      atomicMin(&dq.slot[v], __float_as_uint(one.d2));
      if (MODE == MODE_NORMAL_FOLD) {
        atomicMin(&dq.slot[64u + v], __float_as_uint(one.d2pos));
        if (one.nan) dq.slot[128u + v] = 1u;
      }
    }
  }
  dq.head = (dq.head + take) & 127u;
  dq.n -= take;
  wave_lds_sync();
  if (MODE == MODE_NEAREST_NORMAL) {
    const unsigned long long kk = reinterpret_cast<const unsigned long long*>(dq.slot)[lane];
    if (kk < defer_key<MODE>(best)) { best.d2 = __uint_as_float((uint32_t)(kk >> 32)); best.idx = (uint32_t)(kk >> 1) & 0x7fffffffu; best.pos = (kk & 1ull) == 0ull; }
  } else {
    best.d2 = fminf(best.d2, __uint_as_float(dq.slot[lane]));
    if (MODE == MODE_NORMAL_FOLD) { best.d2pos = fminf(best.d2pos, __uint_as_float(dq.slot[64u + lane])); best.nan |= dq.slot[128u + lane] != 0u; }
  }
}
// The second half of a pre-test batch (defer_pretest, and pretest_consume of the gather-ahead form): the pairs that passed move on to the second
// ring, the exact evaluations'; a full ring is flushed.  Returns true if it was (the lanes' bounds have moved).
template <int MODE>
__device__ __forceinline__ bool pretest_pass_on(const DeviceMesh& mesh, f3 p, DeferQueue& dq, Best<MODE>& best, uint32_t e, bool pass) {
  const unsigned long long rb = __ballot(pass);
  if (rb == 0ull) return false;
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rb, 0u));
  if (pass) dq.q[(dq.head + dq.n + rank) & 127u] = e;
  dq.n += (uint32_t)__popcll(rb);
  if (dq.n < 64u) return false;
  defer_flush<MODE>(mesh, p, dq, best);
  return true;
}
// DEFER = 3: the leaf pre-test run densely too.  It costs the wave its 20 instructions (and a 64-byte scalar load) per leaf triangle
// for the 11 (128^3 x blob-100k) ... 30 (headline) of 64 lanes whose bound reaches the leaf at all — the node test has just said
// which.  Those lanes are queued per leaf triangle (first ring), 64 such pairs are pre-tested at a time — the owner's point and bound
// by lane permutes, the planes by a gather — and the ones that pass move on to the second ring, the exact evaluations' (above).
// Returns true if that ring was flushed (the lanes' bounds have moved).
template <int MODE>
__device__ __forceinline__ bool defer_pretest(const DeviceMesh& mesh, f3 p, float thr, DeferQueue& dq, Best<MODE>& best) {
  const uint32_t lane = threadIdx.x & 63u;
  wave_lds_sync();
  const uint32_t take = min(dq.n1, 64u);
  const bool valid = lane < take;
  const uint32_t e = valid ? dq.q1[(dq.head1 + lane) & 127u] : 0u;
  const uint32_t t = e >> 6, va = owner_addr(e);
  const f3 pv = mk3(owner_fetch(va, p.x), owner_fetch(va, p.y), owner_fetch(va, p.z));
  const float tv = owner_fetch(va, thr);
  const bool pass = valid & !(planes_dist2(pv, mesh.planes[t]) > tv);
  dq.head1 = (dq.head1 + take) & 127u;
  dq.n1 -= take;
  return pretest_pass_on<MODE>(mesh, p, dq, best, e, pass);
}
template <int MODE>
__device__ __forceinline__ void defer_drain(const DeviceMesh& mesh, f3 p, float slack, DeferQueue& dq, Best<MODE>& best) {
  while (dq.n1 != 0u) defer_pretest<MODE>(mesh, p, prune_bound(best.d2, slack), dq, best);
  while (dq.n != 0u) defer_flush<MODE>(mesh, p, dq, best);
}

// GATHER-AHEAD (k_packet's GA form; M2S_GATHER_AHEAD): defer_pretest in two halves, so that the planes' gather — an L2 round trip whose
// addresses are known as soon as the first ring holds 64 pairs — passes under the node tests that follow instead of in front of the plane test.
// pretest_issue reads the 64 ring words (the ring's slots are free again from then on: a pending batch cannot be overrun, whatever the rings'
// size) and requests the four 16-byte pieces of each lane's TriPlanes; pretest_consume, at the next leaf the walk reaches (or when the ring
// fills again inside a long leaf, at the end of the packet's ranges at the latest), takes the owner's point and its bound AS IT IS THEN by lane
// permutes and goes on as defer_pretest does.  The bound a pair is tested against is never older than defer_pretest's, and a batch that waits only
// delays what its evaluations would have told the lanes: pairs, never a result (the argument above DeferLayout).  What is pending lives in 17
// VGPRs that the node loop has to spare and the evaluation body has not: the batch is consumed — its registers dead — before defer_flush runs.
struct PretestAhead {
  TriPlanes tp;      // the lanes' planes, on their way from the issue on
  uint32_t e;        // the lanes' pair words
  bool pending;      // wave-uniform
};
__device__ __forceinline__ void pretest_issue(const DeviceMesh& mesh, DeferQueue& dq, PretestAhead& ga) {   // dq.n1 >= 64
  wave_lds_sync();
  ga.e = dq.q1[(dq.head1 + (threadIdx.x & 63u)) & 127u];
  ga.tp = mesh.planes[ga.e >> 6];
  ga.pending = true;
  dq.head1 = (dq.head1 + 64u) & 127u;
  dq.n1 -= 64u;
}
// After a consume: the 17 registers hold nothing any more, and the compiler is told so (no instruction: an empty definition) — it cannot see that
// `pending` guards them and would otherwise carry them through the evaluation body to the next iteration, which has no room for them.
// This steers the register allocator and nothing checks it but the resource table: after a compiler upgrade, or a change to the walk,
// run tools/kernel_resources.py on this file again — every GA form must show 0 bytes of scratch (without these lines: 52).
__device__ __forceinline__ void pretest_forget(PretestAhead& ga) {
  float* f = reinterpret_cast<float*>(&ga.tp);
  static_assert(sizeof(TriPlanes) == 64, "sixteen words");
  // ONE statement: seventeen separate ones came out with a hazard s_nop between each where the in-leaf consume stands, 16 issue slots a time.
  asm volatile("" : "=v"(f[0]), "=v"(f[1]), "=v"(f[2]), "=v"(f[3]), "=v"(f[4]), "=v"(f[5]), "=v"(f[6]), "=v"(f[7]), "=v"(f[8]), "=v"(f[9]),
                    "=v"(f[10]), "=v"(f[11]), "=v"(f[12]), "=v"(f[13]), "=v"(f[14]), "=v"(f[15]), "=v"(ga.e));
}
// Returns true if the second ring was flushed (the lanes' bounds have moved).
template <int MODE>
__device__ __forceinline__ bool pretest_consume(const DeviceMesh& mesh, f3 p, float thr, DeferQueue& dq, Best<MODE>& best, PretestAhead& ga) {
  const uint32_t e = ga.e, va = owner_addr(e);
  const f3 pv = mk3(owner_fetch(va, p.x), owner_fetch(va, p.y), owner_fetch(va, p.z));
  const float tv = owner_fetch(va, thr);
  const bool pass = !(planes_dist2(pv, ga.tp) > tv);
  ga.pending = false;
  return pretest_pass_on<MODE>(mesh, p, dq, best, e, pass);
}

// (Round 6, measured and not kept — two cursors per wave, so that two record loads are in flight and two node tests issue back to back.  First
// form: idle cursors take the next range of the list or the rest of the other cursor's range; ~100 scalar instructions of bookkeeping per
// iteration; headline walk 7.1 -> 12.6 ms.  Second form: two ranges in lockstep while both last, the same instruction count per node plus ~6
// scalar instructions; 6.47 -> 6.86 ms, 512^3 x sheet-100k Normal 13.3 -> 14.1.  The record loads hit the scalar cache: what a wave waits for
// is its own instruction stream, and at eight waves per SIMD a wave's time follows its instruction count.  profiles/r06_two_cursors_*.)
// The pre-order records [off, end) of the oriented-bound tree for the 64 points of a wave: position wave-uniform (SGPR), node
// records and pre-test planes through scalar loads, a subtree left when no lane's bound reaches it.  BUDGET: the walk may stop
// early (sp.suspended, off = the first record not yet looked at).  EMIT: a suspended walk — surviving subtrees of em.min_bytes ..
// em.max_bytes are written to the next round's list instead of being entered.
// SEEDED: `seed` is the triangle slot (the index space of nr.tri) that the caller has ALREADY evaluated for every lane, ungated — the packet's
// seed; 0xffffffff: none.  The walk passes over that leaf triangle: every fold of Best<MODE> is an idempotent minimum (fminf; two fminf and
// an OR of `nan`; the lexicographic minimum of (d2, index)), so evaluating the seed's arithmetic a second time cannot change a bit, and it
// was what the lanes whose nearest triangle IS the seed did — the pre-test passes for exactly those.  The tree comes from the cut list and
// the seed is k_cut's witness, so the walk always reaches the seed's leaf.  `seed` is wave-uniform (an SGPR).  The split forms (BUDGET, EMIT)
// start from handed-over minima, sit at the SGPR cap and are instantiated without it: their code is what it was.
template <int MODE, bool STATS, bool BUDGET, bool EMIT = false, bool HANDOVER = false, int DEFER = 0, bool GA = false, bool SEEDED = false>
__device__ __forceinline__ void walk_span(const DeviceMesh& mesh, f3 p, float slack, Best<MODE>& best, float& thr, uint32_t& off,
                                          uint32_t end, WalkStats& st, SplitState& sp, EmitState* emp = nullptr, DeferQueue* dqp = nullptr,
                                          PretestAhead* gap = nullptr, uint32_t seed = 0xffffffffu) {
  static_assert(!(SEEDED && (BUDGET || EMIT)), "the split forms pass no seed");
  // The walk addresses NodeExt by BYTE offset (its skip links are stored that way): the scalar loads then take
  // the offset operand directly and the loop carries no address arithmetic.
  // `off` is wave-uniform at every caller (a v_readlane / v_readfirstlane result) and stays so: it only ever takes nr.skip or off + NB.
  // The three outcomes of a visit — pruned, interior, leaf — each set `off` and go on to the loop test.  `below`, the
  // record behind this one, is formed in FRONT of the leaf test because both sides use it (the interior's next record, the start of a leaf's
  // cursor): with the addition on the interior side alone, that side was a block of its own, the join in front of the loop test was compiled
  // through a pair of wave-mask flags, and "add 48 and loop" cost nine scalar instructions and four branches; now six and three.  (An early
  // `continue` for the interior WITHOUT the shared addition moved the gather-ahead batch's 17 registers to other registers inside the leaf and
  // back — 50 more v_mov and 52 bytes of scratch.  profiles/walk_isa.txt.)
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  while (off < end) {
    const NodeExt nr = record_at_bytes<NodeExt>(mesh.ext, off);
    if (STATS) ++st.box;
    const float ed2 = ext_dist2(p, nr);
    if (STATS) st.node_lanes += (uint32_t)__popcll(__ballot(!(ed2 > thr)));
    if (STATS && __ballot(!(ed2 > thr)) == 0ull) {
      ++st.pruned;
      const float vx = p.x - nr.cx, vy = p.y - nr.cy, vz = p.z - nr.cz;
      const float t = nr.nz * vz + nr.ny * vy + nr.nx * vx, sl = fmaxf(fabsf(t - nr.mid) - nr.half, 0.0f);
      if (__ballot(!(sl * sl > thr)) == 0ull) ++st.slab;
      const float rs = __builtin_amdgcn_sqrtf(nr.R * nr.R + (fabsf(nr.mid) + nr.half) * (fabsf(nr.mid) + nr.half));
      const float sq = fmaxf(__builtin_amdgcn_sqrtf(vx * vx + vy * vy + vz * vz) - rs, 0.0f);
      if (__ballot(!(sq * sq > thr)) == 0ull) ++st.sphere;
    }
    if (__ballot(!(ed2 > thr)) == 0ull) { off = nr.skip; continue; }   // a NaN bound keeps the node
    const uint32_t below = off + NB;                            // the first child's record; a leaf's cursor starts there too
    // Which side stands first in the source decides how the register allocator lays the loop out, and the two kinds of form want it differently
    // (tools/kernel_resources.py): the plain forms take the interior visit first — the headline form is 26 scalar instructions and 8 branches
    // shorter that way, statically, most of them in the node loop —, the split forms (BUDGET, EMIT; k_split_round inlines this function three times at the SGPR cap) the leaf, as
    // they always had it: interior first costs k_split_round<1> 16 bytes of scratch more and k_split_round<0> a VGPR.
    if (!(BUDGET || EMIT) && nr.tri < 0) { off = below; continue; }   // interior: on to its first child
    if (nr.tri >= 0) {
      // A leaf.  Its subtree's records [off, nr.skip) are 2 cnt - 1 of them for the cnt triangles nr.tri, nr.tri + 1, ... (a collapsed leaf; cnt = 1: the
      // record alone), so a byte cursor that starts at `below` and steps over two records at a time is at or below nr.skip exactly cnt times, the
      // first time always: leaf_cursor_steps of geo.hip.h, held against cnt = (nr.skip - off + NB) / (2 NB) by
      // tests/test_walk_leaf_count_cpu.py.  No division, no count and no guard in front of the loop.
      uint32_t tri = (uint32_t)nr.tri, cur = below;
      // The seed's leaf (SEEDED).  ONE test per leaf — seed_in_leaf of geo.hip.h: a subtraction, a multiplication, a subtraction, a compare and
      // a branch — is all the node loop pays; the leaf loops below are the same instructions as without a seed.  Where the seed IS one of this
      // leaf's triangles: a single-triangle leaf is passed over; a collapsed leaf is entered like an interior node — the records below it are a
      // tree of their own, every one marked as the (smaller) leaf it would be (bvh.hip: tri = first wherever cnt <= leaf_max) —, so its other
      // triangles are met as leaves of their own and the seed alone is left out.  That costs the node tests on the seed's path, two for a leaf of
      // two triangles, and saves the seed's queued pairs, pre-tests and second evaluations.  Either way the next record is `below`.
      if (SEEDED && seed_in_leaf(seed, tri, below, nr.skip, NB)) {
        // (counted where the walk meets the seed's leaf as the tree has it, not again on the way down inside it)
        if (STATS && !st.seed_inside) { ++st.seed_met; st.seed_lanes += (uint32_t)__popcll(__ballot(!(ed2 > thr))); }
        if (STATS) st.seed_inside = below != nr.skip;
        off = below;
        continue;
      }
      if (DEFER == 3) {
        // GA: the batch pending from an earlier leaf is taken first — one scalar branch per leaf is all the node loop pays —, one issued by
        // this leaf when the ring fills again inside it (long leaves; rare); the ring never holds 128 pairs.
        static_assert(!(GA && (BUDGET || DEFER != 3)), "the gather-ahead form exists for the plain DEFER 3 walk only");
        DeferQueue& dq = *dqp;
        if (GA && gap->pending) {
          if (pretest_consume<MODE>(mesh, p, thr, dq, best, *gap)) thr = prune_bound(best.d2, slack);
          pretest_forget(*gap);
        }
        const bool want = !(ed2 > thr);
        const unsigned long long wb = __ballot(want);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(wb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wb, 0u));
        const uint32_t wn = (uint32_t)__popcll(wb);
        // This lane's ring slot as a byte offset, formed once per leaf; per triangle it moves on by the wn pairs just queued (one add, the mask at
        // the store) and the pair word by one triangle.  A batch taken out of the ring (head1 + 64, n1 - 64) leaves head1 + n1 where it was.
        // (Measured and not kept: no exec region around the store — the lanes that do not want the leaf all write the free slot BEHIND the wn wanted
        // ones, two scalar instructions fewer per triangle.  64 - wn lanes storing to one address are not free: headline distance 6.110 -> 6.136 ms,
        // 512^3 x blob-1M 17.20 -> 17.32.  profiles/walk_diet_ab.txt, series 1.)
        uint32_t slot4 = (dq.head1 + dq.n1 + rank) << 2, pair = (threadIdx.x & 63u) | (tri << 6);
        const uint32_t step4 = wn << 2;
        do {
          if (want) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(dq.q1) + (slot4 & 0x1fcu)) = pair;
          slot4 += step4;
          pair += 64u;
          dq.n1 += wn;
          if (BUDGET) ++sp.units;
          if (dq.n1 >= 64u) {
            if (BUDGET) sp.units += 4u;
            if (GA) {
              if (gap->pending) {
                if (pretest_consume<MODE>(mesh, p, thr, dq, best, *gap)) thr = prune_bound(best.d2, slack);
                pretest_forget(*gap);
              }
              pretest_issue(mesh, dq, *gap);
            } else if (defer_pretest<MODE>(mesh, p, thr, dq, best)) thr = prune_bound(best.d2, slack);
          }
          cur += 2u * NB;
        } while (cur <= nr.skip);
      } else
      do {
        if (STATS && tri == st.seed) {   // (the walk has not passed over the seed — M2S_SEED_SKIP=0: what becomes of it)
          const bool want = !(ed2 > thr);
          ++st.seed_met;
          st.seed_lanes += (uint32_t)__popcll(__ballot(want));
          st.seed_passed += (uint32_t)__popcll(__ballot(want & !(planes_dist2(p, record_at(mesh.planes, tri)) > thr)));
        }
        if (STATS) { ++st.ext; st.pre_lanes += (uint32_t)__popcll(__ballot(!(ed2 > thr))); }
        if (BUDGET) ++sp.units;
        const TriPlanes tp = record_at(mesh.planes, tri);   // scalar: small, needed for every leaf triangle
        const bool reach = !(planes_dist2(p, tp) > thr);
        const unsigned long long rb = __ballot(reach);
        if (rb != 0ull) {   // some lane's bound reaches the triangle itself
          if (STATS) { ++st.leaf; st.pairs += (uint32_t)__popcll(rb); }
          if (DEFER != 0 && !(DEFER == 2 && (uint32_t)__popcll(rb) >= DEFER_DIRECT_LANES)) {
            DeferQueue& dq = *dqp;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rb, 0u));
            if (reach) dq.q[(dq.head + dq.n + rank) & 127u] = (threadIdx.x & 63u) | (tri << 6);
            dq.n += (uint32_t)__popcll(rb);
            if (dq.n >= 64u) {
              if (BUDGET) sp.units += 4u;
              defer_flush<MODE>(mesh, p, dq, best);
              thr = prune_bound(best.d2, slack);
            }
          } else {
            if (BUDGET) sp.units += 4u;
            const TriRec tr = record_at_vec(mesh.tris, tri);
            eval_triangle_leaf<MODE>(best, p, tr, reach);
            thr = prune_bound(best.d2, slack);
          }
        }
        ++tri;
        cur += 2u * NB;
      } while (cur <= nr.skip);
      off = nr.skip;
      if (BUDGET) {
        sp.units += 3u;                                           // (+ 1 per leaf triangle, counted above: 3 + cnt as ever, looked at here only)
        if (sp.units >= sp.next_check) {
          // (no exit of its own: a second way out of this loop cost the walk 11 % although it was never taken; the loop ends by its
          // own condition)
          bool go;
          if (HANDOVER) go = split_stragglers_only(sp);                   // k_packet: measured patience
          else {                                                           // a follow-up round: `grace` units after the flag was first seen up
            go = sp.flag_seen;
            if (!go && split_peek(sp.flag_addr) != 0u) { sp.flag_seen = true; sp.next_check = sp.units + sp.grace; }
          }
          if (go) {
            // Suspended.  No exit of its own and nothing but three scalar moves here: the loop ends by its condition (and so does the
            // caller's loop over the ranges, whose count is taken away).  Every other form tried in k_packet — an early return, a
            // hand-over in this branch that ends the wave, a retry loop around the call, a rewound range counter — cost the 512^3
            // walk 10 ... 40 % although none of it was ever executed there.
            if (off < end || HANDOVER) { sp.suspended = true; sp.resume_end = end; end = off; if (HANDOVER) *sp.n_ranges = 0u; }
            sp.next_check = 0xffffffffu;
          } else if (HANDOVER || !sp.flag_seen) {
            sp.next_check = sp.units + SPLIT_CHECK_EVERY;
          }
        }
      }
      continue;
    }
    // (the split forms' interior visit)
    if (EMIT) {
      EmitState& em = *emp;
      const uint32_t bytes = nr.skip - off;
      if (bytes >= em.min_bytes && bytes <= em.max_bytes) {
        if (em.used == em.room) emit_reserve(em);
        if (em.used < em.room) {
          if ((threadIdx.x & 63u) == 0u) em.list[em.base + em.used] = make_uint4(em.packet, off, nr.skip, em.slot);
          ++em.used;
          off = nr.skip;                                      // somebody else's from here
          continue;
        }
      }
    }
    off = below;
  }
}

// The value of one voxel / query, stored the way the call's delivery asks for (plain, peer stores, trailing push).
__device__ __forceinline__ void store_grid_result(float* __restrict__ out, size_t out_index, float result, bool store, const GridParams& g,
                                                  const GridBrick& vox, const PeerOut& peers, int lane) {
  if (peers.progress != nullptr) {
    // M2S_PEER_TRAIL: the copy kernel that trails this walk runs on other XCDs, whose L2s are separate.  The values are
    // stored write-through at device scope (no L2 write-back fence: a release fence per wave — buffer_wbl2 — made the walk ten
    // times slower), the wave waits until the store has been acknowledged, and only then counts the packet.
    if (store) __hip_atomic_store(&out[out_index], result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // one counter per (unit, brick row): thousands of device-scope atomics on ONE address serialise at the memory side
    // and the packet that completes a row counts the row on the unit's own counter, the only address the copy kernel polls
    if (lane == 0) {
      const uint32_t unit = vox.bx >> peers.unit_log;
      const uint32_t nbx = bricks_along(g.xe - g.xb, g.bl[0]), nbz = g.nbz;
      const uint32_t bricks = min((unit + 1u) << peers.unit_log, nbx) - (unit << peers.unit_log);
      const uint32_t old = __hip_atomic_fetch_add(&peers.progress[peers.units + unit * peers.rows + vox.by], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old + 1u == bricks * nbz) __hip_atomic_fetch_add(&peers.progress[unit], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (store) out[out_index] = result;
  // M2S_PEER_STORE: the same value into every peer's whole-grid buffer (indices are whole-grid there)
  if (peers.n != 0u && store) {
    const size_t gi = out_index + (size_t)g.out_off;
    for (uint32_t i = 0; i < peers.n; ++i) peers.p[i][gi] = result;
  }
}

// ---- k_packet -------------------------------------------------------------------------------
// `seed_in` (one TriRec slot per 2^seed_shift bricks per axis, may be null) replaces the greedy descent:
// the packet starts from a triangle near its own centre (jump-flooding seed pass, seeds.hip).
// (eight waves per SIMD: the split variant's bookkeeping would otherwise take the kernel to 106 SGPRs — seven waves, - 12 %; the
// compiler parks what does not fit in spare VGPR lanes)
// GA (DEFER 3 only): the queued pre-tests' gathers issued ahead of their use (PretestAhead).
template <bool GRID, int MODE, int SIGN, bool STATS, bool SPLIT, int DEFER = 0, bool GA = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_packet(DeviceMesh mesh, GridParams g, const float4* __restrict__ qsorted,
                                               const uint32_t* __restrict__ perm, uint32_t n_q,
                                               const uint32_t* __restrict__ plane, float* __restrict__ out,
                                               int* __restrict__ err, uint32_t n_packets,
                                               const uint32_t* __restrict__ seed_in, uint32_t seed_shift,
                                               uint32_t seed_ny, uint32_t seed_nz,
                                               const GridParams* __restrict__ seed_lattice, CutList cut, PeerOut peers, SplitCtl split) {
  const int lane = threadIdx.x & 63;
  // the first and the last workgroup an XCD is handed stamp the time: start of the launch there; from here on its wave slots fall idle
  if (SPLIT && (blockIdx.x < 8u || blockIdx.x + 8u >= gridDim.x) && lane == 0) {
    const uint32_t t = split.idle_below /* forced */ ? 0u : split_now();
    if (blockIdx.x < 8u) split_poke(split_flag_addr(split, 0u) + 8, t);
    if (blockIdx.x + 8u >= gridDim.x) split_poke(split_flag_addr(split, 0u), t | 1u);
  }
  const uint32_t block = xcd_remap(blockIdx.x);
  // wave-uniform, and said so: the brick decode below (two divisions by multiplication, shifts, bounds) then runs on the scalar unit
  const uint32_t packet = (uint32_t)__builtin_amdgcn_readfirstlane((int)block);   // one packet per single-wave workgroup: the slot is free as soon as the walk ends (4 waves per group: +3.8 %)
  if (packet >= n_packets) return;

  f3 p;
  size_t out_index;
  bool store;
  GridBrick vox{};
  if (GRID) {
    vox = grid_lane_voxel(g, packet, lane);
    if (!vox.brick_in_grid) return;      // padding of the super-brick order
    p = grid_point(g, vox);
    out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;
    store = vox.in_range;
  } else {
    // generic queries: `plane` carries the packet table of launch_query_distance (k_qcells): [0] packets, [1] mode, [2 + k] the
    // first sorted query of packet k.  mode 1 (more packets than the launch has waves): 64 consecutive queries per packet.
    uint32_t first, cnt;
    if (!query_packet_range(plane, packet, n_q, &first, &cnt)) return;
    const uint32_t i = first + min((uint32_t)lane, cnt - 1u);
    const float4 q = qsorted[i];
    p = mk3(q.x, q.y, q.z);
    out_index = perm[i];
    store = (uint32_t)lane < cnt;
  }

  Best<MODE> best;
  WalkStats st;
  uint32_t st_ranges = 0, st_band = 0, st_rbytes = 0;
  if (mesh.n_nodes) {
    // Placement of the headline form's node loop.  The prologue below lost 960 bytes when the call's constants moved to the host, and the
    // node loop of walk_span — the same instructions as before — came to start 16 bytes into a 64-byte line of the instruction cache
    // instead of 36: the headline still gained (distance 6.42 -> 6.31 ms) but 512^3 x blob-1M, whose packets spend 2.8 times as long in
    // that loop, LOST 0.5 % (17.78 -> 17.85 ms).  Twelve bytes of padding put the loop back at 36: 6.42 -> 6.29 and 17.78 -> 17.65 ms, same
    // box, alternating runs (profiles/prologue_ab.txt).  A change of the code in front of the loop moves it again: tools/isa_kernel_diff.py
    // shows the change, llvm-objdump -d the loop's address (the backward branch over ~1 860 bytes), and the two configs decide.
    // (Side effect, part of what was measured: behind an asm statement the compiler reads mesh_scale — a global load, "may be clobbered" —
    // through the vector unit, one VMEM instruction more per packet; the seed index and the records stay scalar loads.)
    // Decided again when the node loop's bookkeeping was trimmed and the loop moved: with the three s_nop its loop test (three instructions in
    // front of the record load, where the backward branches land) stood at byte 8 of a line and the load at byte 20.  Measured, loop test at byte 52
    // of the line before / 60 / 8 / 24 / 36 by no asm statement at all, 0, 3, 7 and 10 s_nop: headline distance 6.154 / 6.186 / 6.137 / 6.136 / 6.137 ms,
    // 512^3 x blob-1M 17.32 / 17.34 / 17.20 / 17.17 / 17.16 (parent 6.263 and 17.62; profiles/walk_diet_ab.txt, series 2).  A record load in the first
    // bytes of a line costs blob-1M 0.7 %; ten s_nop put the loop test back at byte 36, where it has stood since the padding was introduced.
    // Among 3, 7 and 10 s_nop nothing is measured to matter (the headline is level; blob-1M's 0.04 ms between 3 and 10 is one series of four
    // runs, two of its spreads): what IS measured is that the load must not stand in the first bytes of a line.  Ten are seven issue slots per
    // packet more than three; the position the parent had was kept so that the A/B against it compares the loop and not its placement.
    if (GRID && MODE == MODE_UNSIGNED && SIGN == SIGN_GRID_PLANE && DEFER == 3 && GA) asm volatile(".rept 5\n s_nop 0\n .endr");
    const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
    SplitState sp;
    if (SPLIT) split_arm(sp, split, 0u, true);
    __shared__ unsigned long long defer_lds[DEFER ? DeferLayout<MODE>::DWORDS : 1];
    DeferQueue dq = {nullptr, nullptr, 0u, 0u};
    if (DEFER) dq = defer_begin<MODE>(defer_lds);
    PretestAhead ga;
    ga.pending = false;

    // pre-order ranges to walk: the brick's cut list (grid path), or the whole tree.  The list is 64 bytes that nobody has
    // touched before (written by k_cut, read once), and the seed is a chain of two more cold loads (its index, then its record).
    // The list word is REQUESTED here and first USED behind the seed evaluation: nothing in between reads it, so the compiler's
    // s_waitcnt vmcnt(0) stands at the decode below and the list's miss passes under the seed chain and its ~140 instructions.
    // (Decoded right here, as it was, the wait stood directly behind the load, in front of the seed's loads: three misses in a row.)
    constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
    uint32_t cw = 0;
    uint32_t n_ranges = 1, cut_off_v = 0, cut_end_v = (lane == 1) ? mesh.n_nodes * NB : 0u;   // no list: lane 1 holds the whole tree
    if (SPLIT) sp.n_ranges = &n_ranges;
    // generic queries: the packet's centre (its seed cell below) is a vector load too.  Requested in FRONT of the list word: vmcnt counts
    // in order, so the seed chain can then wait for the centre alone (behind the list word it would wait for both).
    float4 centre = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!GRID && seed_in != nullptr && cut.centres != nullptr) centre = cut.centres[packet];
    if (cut.lists != nullptr) {
      const uint32_t cb = GRID ? __builtin_amdgcn_readfirstlane((((vox.bx + cut.bx_off) >> cut.log) * cut.ny + (vox.by >> cut.log)) * cut.nz + (vox.bz >> cut.log))
                               : packet;
      // The whole 64-byte record with ONE vector load — lane l takes word l.
      cw = cut.lists[(size_t)cb * CUT_WORDS + ((uint32_t)lane & 15u)];
    }
    // The slot of the triangle evaluated here for every lane: the walk passes over it (walk_span SEEDED).  The launch's word (SplitCtl::plain_seed_none)
    // is 0xffffffff where it shall not (M2S_SEED_SKIP=0) — ORed in, the slot becomes "none", the parent's walk — and 0 where it shall.
    uint32_t seed_slot = 0xffffffffu;
    if (seed_in != nullptr) {
      // seed: a triangle near this packet's centre, from the seed pass
      uint32_t sidx = packet;
      if (GRID) {  // 2^seed_shift bricks per axis share one seed point
        sidx = (((vox.bx + cut.bx_off) >> seed_shift) * seed_ny + (vox.by >> seed_shift)) * seed_nz + (vox.bz >> seed_shift);
      } else {     // generic queries: the lattice cell that holds the packet's centre (its first point without the packet boxes)
        const GridParams L = *seed_lattice;
        float q0[3] = {__shfl(p.x, 0), __shfl(p.y, 0), __shfl(p.z, 0)};
        if (cut.centres != nullptr) {      // the same cell k_cut<false> took this packet's seed from
          q0[0] = centre.x; q0[1] = centre.y; q0[2] = centre.z;
        }
        sidx = query_lattice_cell_uniform(L, q0[0], q0[1], q0[2]);
      }
      // one seed per packet: wave-uniform, so the 96-byte record comes through scalar loads
      const uint32_t slot = __builtin_amdgcn_readfirstlane(min(seed_in[sidx], mesh.n_tris - 1));
      const TriRec tr = record_at(mesh.tris, slot);
      eval_triangle<MODE>(best, p, tr);
      seed_slot = slot;
    } else {
      // seed: greedy descent towards the packet's first point, evaluate that leaf for every lane
      const f3 c = {__shfl(p.x, 0), __shfl(p.y, 0), __shfl(p.z, 0)};
      uint32_t n = 0;
      NodeRec nr = mesh.nodes[0];
      while (nr.tri < 0) {
        const uint32_t l = n + 1;
        const NodeRec nl = mesh.nodes[l];
        const uint32_t r = nl.skip;
        const NodeRec nrr = mesh.nodes[r];
        const float dl = box_dist2(c, nl.mnx, nl.mny, nl.mnz, nl.mxx, nl.mxy, nl.mxz);
        const float dr = box_dist2(c, nrr.mnx, nrr.mny, nrr.mnz, nrr.mxx, nrr.mxy, nrr.mxz);
        const bool go_left = __builtin_amdgcn_readfirstlane((int)(dl <= dr)) != 0;
        n = go_left ? l : r;
        nr = go_left ? nl : nrr;
      }
      const TriRec tr = mesh.tris[nr.tri];
      eval_triangle<MODE>(best, p, tr);
      seed_slot = (uint32_t)__builtin_amdgcn_readfirstlane(nr.tri);   // (the descent is wave-uniform: towards lane 0's point)
    }
    if (STATS) st.seed = seed_slot;
    if (!SPLIT) seed_slot |= split.plain_seed_none;
    if (cut.lists != nullptr) {
      // The list word's first use.  Lanes 1..15 decode their range side by side (eight VALU instructions for the whole list), and the
      // range loop below fetches (start, end) of range k from lane 1 + k with two v_readlane: no load and no scalar arithmetic per range.
      // (Decoding on the scalar unit, one range at a time, cost the Normal-sign walk of 1024^3 1.3 %: 9 SALU x ~10 ranges per packet.)
      const uint32_t cS = cut.start_bits, cfirst = cw & ((1u << cS) - 1u);
      const uint32_t clen = ((cw >> cS) & ((1u << (27u - cS)) - 1u)) << (cw >> 27);
      cut_off_v = cfirst * NB;
      cut_end_v = min(cfirst + clen, mesh.n_nodes) * NB;
      n_ranges = __builtin_amdgcn_readfirstlane(cw);
    }

    float thr = prune_bound(best.d2, slack);
    if (STATS && GRID) {
      const float cells = __shfl(__builtin_amdgcn_sqrtf(best.d2), 0) / fabsf(g.size[0]);
      st_band = cells < 1.0f ? 0u : min(7u, 1u + (uint32_t)__builtin_amdgcn_readfirstlane((int)floorf(log2f(cells))));
      st_band = __builtin_amdgcn_readfirstlane(st_band);
    }
    // M2S_STATS=2: a second, counting-only traversal that starts from the final bound ("perfect seed")
    const int passes = (STATS && mesh.stats != nullptr && mesh.stats[7] == 2ull) ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
      if (pass == 1) { st.box = 0; st.ext = 0; st.leaf = 0; }
      if (STATS) st_ranges = n_ranges;
      uint32_t range = 0, off = 0;
      for (; range < n_ranges; ++range) {
        // (a rounded-up range may reach into the next one: those records are then walked twice, which changes no minimum)
        off = (uint32_t)__builtin_amdgcn_readlane((int)cut_off_v, (int)(1u + range));
        const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)cut_end_v, (int)(1u + range));
        if (STATS) st_rbytes += end - off;
        walk_span<MODE, STATS, SPLIT, false, SPLIT, DEFER, GA, !SPLIT>(mesh, p, slack, best, thr, off, end, st, sp, nullptr, &dq, &ga, seed_slot);
      }
      // (a batch still pending: with the bound the walk ended on, as defer_drain's own)
      if (GA && ga.pending) pretest_consume<MODE>(mesh, p, prune_bound(best.d2, slack), dq, best, ga);
      if (DEFER) defer_drain<MODE>(mesh, p, slack, dq, best);   // what is still queued (a suspended packet hands over complete minima)
      if (SPLIT && sp.suspended) {
        // (range has been stepped once more by the loop's increment)
        if (!split_handover<MODE>(split, packet, range - 1u, off, best, err)) atomicOr(err, ERRF_SPLIT_OVERFLOW);   // cannot happen: a slot per packet
        return;                                                                // k_split_finish writes this packet's voxels
      }
    }
  }

  if (STATS && mesh.stats != nullptr && lane == 0) {
    atomicAdd(&mesh.stats[0], (unsigned long long)st.box);
    atomicAdd(&mesh.stats[1], (unsigned long long)st.ext);
    atomicAdd(&mesh.stats[2], (unsigned long long)st.leaf);
    atomicAdd(&mesh.stats[3], 1ull);
    atomicAdd(&mesh.stats[4], (unsigned long long)st.pruned);
    atomicAdd(&mesh.stats[5], (unsigned long long)st.slab);
    atomicAdd(&mesh.stats[6], (unsigned long long)st.sphere);
    atomicMax(&mesh.stats[72], (unsigned long long)st.box);
    atomicMax(&mesh.stats[73], (unsigned long long)st.leaf);
    atomicMax(&mesh.stats[74], (unsigned long long)(st.box + st.ext + 4u * st.leaf));
    atomicAdd(&mesh.stats[75], (unsigned long long)st.node_lanes);
    atomicAdd(&mesh.stats[76], (unsigned long long)st.pre_lanes);
    atomicAdd(&mesh.stats[77], (unsigned long long)st.pairs);
    atomicAdd(&mesh.stats[78], (unsigned long long)st.seed_lanes);
    atomicAdd(&mesh.stats[79], (unsigned long long)st.seed_passed);
    atomicAdd(&mesh.stats[120], (unsigned long long)st.seed_met);
    unsigned long long* q = mesh.stats + 8 + 8 * st_band;
    atomicAdd(&q[0], (unsigned long long)st.box);
    atomicAdd(&q[1], (unsigned long long)st.ext);
    atomicAdd(&q[2], (unsigned long long)st.leaf);
    atomicAdd(&q[3], 1ull);
    atomicAdd(&q[4], (unsigned long long)st_ranges);
    atomicAdd(&q[5], (unsigned long long)st.pairs);
    atomicAdd(&q[6], (unsigned long long)st_rbytes);
    atomicAdd(&q[7], (unsigned long long)(st_rbytes <= 4096u ? 1u : 0u));
    // histogram of the packets' work units (node tests + pre-tests + 4 x exact evaluations) in octaves: stats[80 + log2]
    const uint32_t units = st.box + st.ext + 4u * st.leaf;
    // (octaves 0..23: the words from stats[104] on are k_cut's visit counters)
    atomicAdd(&mesh.stats[80 + min(31u - (uint32_t)__builtin_clz(units | 1u), 23u)], 1ull);
  }

  bool negate = false;
  if (MODE == MODE_UNSIGNED) {
    if (SIGN == SIGN_GRID_PLANE) {
      const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
      negate = (plane[w] >> (vox.z & 31u)) & 1u;                       // grid.rs:630-636
    } else if (SIGN == SIGN_RAYS3) {
      // best of three (bvh.rs:131-141, rtree_bvh.rs:161-171): where the +X and +Y parities agree they ARE the majority, so the +Z
      // walk only runs for a packet in which some lane's first two rays disagree (never, for a watertight mesh, but for rays
      // through an edge; 10 M queries x blob-100k: a third of the 2 ms of stabbing).  The vote's result is the same.
      __shared__ uint32_t ray_lds[DEFER != 0 ? 192 : 1];
      const uint32_t cx = DEFER != 0 ? stab_count_dense<0>(mesh, p, ray_lds) : stab_count<0>(mesh, p);
      const uint32_t cy = DEFER != 0 ? stab_count_dense<1>(mesh, p, ray_lds) : stab_count<1>(mesh, p);
      uint32_t cz = cx;
      if (__ballot(((cx ^ cy) & 1u) != 0u) != 0ull) cz = DEFER != 0 ? stab_count_dense<2>(mesh, p, ray_lds) : stab_count<2>(mesh, p);
      negate = ((cx & 1u) + (cy & 1u) + (cz & 1u)) > 1u;
    }
  }
  if (MODE == MODE_NORMAL_FOLD && best.nan) atomicOr(err, ERRF_NAN);
  const float result = finish<MODE>(best, negate);
  if (GRID) store_grid_result(out, out_index, result, store, g, vox, peers, lane);
  else if (store) out[out_index] = result;
}

// ---- packet groups: several waves per packet (round 6) ------------------------------------------------------------------------
// A launch shallower than the chip (64^3 ... 128^3 over 100 k triangles: 4 096 ... 32 768 packets on 8 192 wave slots, triangles much finer
// than the bricks) lasts as long as its slowest packet's chain of dependent loads — 0.58 - 0.64 ms whatever the grid (round 5) — while
// most wave slots idle.  Here a packet is a workgroup of GROUP_WAVES = 2 or 4 waves: every wave evaluates the packet's seed, then walks its share
// of the tree — the subtrees w, w + GROUP_WAVES, ... of the TOP_SUBTREES subtrees TOP_LOG levels below the root (k_tree_top; neighbours
// in Morton order go to different waves, so the part of the mesh next to the brick is dealt out evenly) — with its own queues but ONE
// set of per-voxel minima in LDS: the queued evaluations fold into them with atomic minima (as they always did) and every wave refreshes
// its bounds from them after each batch, so a wave prunes with what the others have found.  A minimum is a minimum: the same bits as
// one wave walking everything (parity suite in this form too).  Grid calls without cut lists and without the split walk, leaf work fully
// queued (DEFER = 3).  Walk, one wave / group (profiles/r06_groups.txt): blob-100k 32^3 1.22 -> 0.46 ms, 48^3 0.87 -> 0.42, 64^3 0.66 -> 0.50, 80^3 0.56 ->
// 0.49, 96^3 0.62 -> 0.55; blob-11k 32^3 0.30 -> 0.12, 64^3 0.23 -> 0.14.  More waves do not keep helping — every wave starts from the seed's bound
// alone and learns what the others found only batch by batch, so the group's total work grows: 16 waves at 32^3 0.56 ms, 8 at 64^3 0.59 — and
// from ~110^3 on (four rounds of the chip's wave slots) one wave per packet is faster again.
constexpr uint32_t GROUP_MAX_WAVES = 4, TOP_LOG = 8, TOP_SUBTREES = 1u << TOP_LOG;   // 2 or 4 waves per packet, chosen by the launch (blockDim.x / 64)
__global__ __launch_bounds__(TOP_SUBTREES) void k_tree_top(DeviceMesh mesh, uint2* __restrict__ top) {
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  const uint32_t sub = threadIdx.x;
  uint32_t off = 0, end = mesh.n_nodes * NB;
  for (uint32_t lv = 0; lv < TOP_LOG && off < end; ++lv) {
    const NodeExt* nr = reinterpret_cast<const NodeExt*>(reinterpret_cast<const char*>(mesh.ext) + off);
    const uint32_t rest = sub & ((1u << (TOP_LOG - lv)) - 1u);
    if (nr->tri >= 0) { if (rest != 0u) end = off; break; }      // a leaf on the way belongs to the subtree whose remaining bits are zero
    const uint32_t skip = nr->skip, left = off + NB;
    const uint32_t right = reinterpret_cast<const NodeExt*>(reinterpret_cast<const char*>(mesh.ext) + left)->skip;
    if ((sub >> (TOP_LOG - 1u - lv)) & 1u) { off = right; end = skip; } else { off = left; end = right; }
  }
  top[sub] = make_uint2(off, end);
}
template <int MODE, int SIGN>
__global__ __launch_bounds__(64 * GROUP_MAX_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_packet_group(
    DeviceMesh mesh, GridParams g, const uint32_t* __restrict__ plane, float* __restrict__ out, int* __restrict__ err, uint32_t n_packets,
    const uint32_t* __restrict__ seed_in, uint32_t seed_shift, uint32_t seed_ny, uint32_t seed_nz, uint32_t bx_off, const uint2* __restrict__ top, PeerOut peers,
    uint32_t seed_none) {   // 0: the walks pass over the seed's leaf triangle, 0xffffffff: they evaluate it again (k_packet)
  static_assert(MODE == MODE_UNSIGNED || MODE == MODE_NORMAL_FOLD, "grid modes");
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t packet = (uint32_t)__builtin_amdgcn_readfirstlane((int)xcd_remap(blockIdx.x));
  if (packet >= n_packets) return;
  const GridBrick vox = grid_lane_voxel(g, packet, lane);
  if (!vox.brick_in_grid) return;        // padding of the super-brick order (the same for every wave of the group)
  const f3 p = grid_point(g, vox);
  const size_t out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;

  extern __shared__ unsigned long long group_lds[];   // blockDim.x / 64 x 256 ring words, then DeferLayout<MODE>::SLOT_WORDS slot words
  const uint32_t GROUP_WAVES = blockDim.x >> 6;
  uint32_t* const lds = reinterpret_cast<uint32_t*>(group_lds);
  DeferQueue dq = {lds + wave * 256u, lds + GROUP_WAVES * 256u, 0u, 0u, lds + wave * 256u + 128u, 0u, 0u};   // own rings, shared minima
  if (wave == 0u) {
    dq.slot[lane] = 0x7f800000u;
    if (MODE == MODE_NORMAL_FOLD) { dq.slot[64 + lane] = 0x7f800000u; dq.slot[128 + lane] = 0u; }
  }
  Best<MODE> best;
  if (mesh.n_nodes) {
    const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
    uint32_t slot = 0;
    if (seed_in != nullptr) {
      const uint32_t sidx = (((vox.bx + bx_off) >> seed_shift) * seed_ny + (vox.by >> seed_shift)) * seed_nz + (vox.bz >> seed_shift);
      slot = __builtin_amdgcn_readfirstlane(min(seed_in[sidx], mesh.n_tris - 1));
    }
    eval_triangle<MODE>(best, p, record_at(mesh.tris, slot));
    float thr = prune_bound(best.d2, slack);
    __syncthreads();                     // the shared minima are initialised
    WalkStats st;
    SplitState sp;
    for (uint32_t k = wave; k < TOP_SUBTREES; k += GROUP_WAVES) {
      const uint2 r = top[k];            // wave-uniform
      uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.x);
      const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y);
      if (off >= end) continue;
      walk_span<MODE, false, false, false, false, 3, false, true>(mesh, p, slack, best, thr, off, end, st, sp, nullptr, &dq, nullptr, slot | seed_none);
    }
    defer_drain<MODE>(mesh, p, slack, dq, best);
    // this wave's minima (the seed's among them) join the group's
    atomicMin(&dq.slot[lane], __float_as_uint(best.d2));
    if (MODE == MODE_NORMAL_FOLD) {
      atomicMin(&dq.slot[64 + lane], __float_as_uint(best.d2pos));
      if (best.nan) dq.slot[128 + lane] = 1u;
    }
    __syncthreads();
    if (wave != 0u) return;
    best.d2 = __uint_as_float(dq.slot[lane]);
    if (MODE == MODE_NORMAL_FOLD) { best.d2pos = __uint_as_float(dq.slot[64 + lane]); best.nan = dq.slot[128 + lane] != 0u; }
  } else if (wave != 0u) return;

  bool negate = false;
  if (MODE == MODE_UNSIGNED && SIGN == SIGN_GRID_PLANE) {
    const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
    negate = (plane[w] >> (vox.z & 31u)) & 1u;                       // grid.rs:630-636
  }
  if (MODE == MODE_NORMAL_FOLD && best.nan) atomicOr(err, ERRF_NAN);
  store_grid_result(out, out_index, finish<MODE>(best, negate), vox.in_range, g, vox, peers, lane);
}

// One follow-up round of the split walk (grid path): a fixed set of single-wave workgroups strides the round's list.  An item is either
// a CONTINUATION — a suspended packet: the rest of its range `range` from record `first` on, and the ranges behind it (round 1) — or a
// subtree [first, end) that a suspended walk did not enter.  The wave rebuilds the packet's 64 points, starts from the slot's current
// minima (plain loads: a stale value is merely a looser bound), walks, and folds what it found into the slot.  A continuation is walked
// in emit mode from the start; a subtree may be suspended in its turn (except in the last round, `final`) and is then finished in emit
// mode: what is not entered goes to the next round's list.
template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_split_round(DeviceMesh mesh, GridParams g, SplitCtl split, CutList cut, uint32_t round, bool final, int* __restrict__ err) {
  constexpr uint32_t AW = MODE == MODE_NORMAL_FOLD ? 128u : 64u;
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  const int lane = threadIdx.x & 63;
  const uint32_t n_items = min(split.cnt[1u + round], split.cap_items);
  const uint4* list = split.items + (size_t)(round - 1u) * split.cap_items;
  for (uint32_t i = blockIdx.x; i < n_items; i += gridDim.x) {
    const uint4 it = list[i];
    const uint32_t packet = __builtin_amdgcn_readfirstlane(it.x), third = __builtin_amdgcn_readfirstlane(it.z), tag = __builtin_amdgcn_readfirstlane(it.w);
    const uint32_t slot = tag & ~SPLIT_CONTINUATION;
    const bool continuation = (tag & SPLIT_CONTINUATION) != 0u;
    uint32_t off = __builtin_amdgcn_readfirstlane(it.y);
    if (!continuation && off >= third) continue;                           // an empty item (the unused part of a reserved block)
    const GridBrick vox = grid_lane_voxel(g, packet, lane);
    const f3 p = grid_point(g, vox);
    const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
    uint32_t* acc = split.acc + (size_t)slot * AW;
    Best<MODE> best;
    const uint32_t d2_in = acc[lane];
    uint32_t d2pos_in = 0x7f800000u;
    best.d2 = __uint_as_float(d2_in);
    if (MODE == MODE_NORMAL_FOLD) { d2pos_in = acc[64 + lane]; best.d2pos = __uint_as_float(d2pos_in); }
    float thr = prune_bound(best.d2, slack);
    WalkStats st;
    SplitState idle;
    EmitState em;
    __shared__ unsigned long long defer_lds[DeferLayout<MODE>::DWORDS];
    wave_lds_sync();                                                         // (the previous item's slots have been read)
    DeferQueue dq = defer_begin<MODE>(defer_lds);
    if (continuation) {
      // the packet's ranges again (k_packet's decode), from range `third` on
      uint32_t n_ranges = 1, cut_off_v = 0, cut_end_v = (lane == 1) ? mesh.n_nodes * NB : 0u;
      if (cut.lists != nullptr) {
        const uint32_t cb = __builtin_amdgcn_readfirstlane((((vox.bx + cut.bx_off) >> cut.log) * cut.ny + (vox.by >> cut.log)) * cut.nz + (vox.bz >> cut.log));
        const uint32_t cw = cut.lists[(size_t)cb * CUT_WORDS + ((uint32_t)lane & 15u)];
        const uint32_t cS = cut.start_bits, cfirst = cw & ((1u << cS) - 1u);
        const uint32_t clen = ((cw >> cS) & ((1u << (27u - cS)) - 1u)) << (cw >> 27);
        cut_off_v = cfirst * NB;
        cut_end_v = min(cfirst + clen, mesh.n_nodes) * NB;
        n_ranges = __builtin_amdgcn_readfirstlane(cw);
      }
      if (!final) emit_begin(em, split, round + 1u, packet, slot);           // (a one-round configuration walks everything here)
      for (uint32_t range = third; range < n_ranges; ++range) {
        if (range != third) off = (uint32_t)__builtin_amdgcn_readlane((int)cut_off_v, (int)(1u + range));
        const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)cut_end_v, (int)(1u + range));
        walk_span<MODE, false, false, true, false, 3>(mesh, p, slack, best, thr, off, end, st, idle, &em, &dq);
      }
      emit_close(em);
    } else {
      SplitState sp;
      split_arm(sp, split, round, !final);
      walk_span<MODE, false, true, false, false, 3>(mesh, p, slack, best, thr, off, third, st, sp, nullptr, &dq);
      if (sp.suspended) {
        emit_begin(em, split, round + 1u, packet, slot);
        walk_span<MODE, false, false, true, false, 3>(mesh, p, slack, best, thr, off, sp.resume_end, st, idle, &em, &dq);
        emit_close(em);
      }
    }
    defer_drain<MODE>(mesh, p, slack, dq, best);
    // NaN never enters a minimum (fminf drops it), so the words stay ordered like non-negative floats
    if (__float_as_uint(best.d2) < d2_in) atomicMin(&acc[lane], __float_as_uint(best.d2));
    if (MODE == MODE_NORMAL_FOLD) {
      if (__float_as_uint(best.d2pos) < d2pos_in) atomicMin(&acc[64 + lane], __float_as_uint(best.d2pos));
      if (best.nan) atomicOr(err, ERRF_NAN);
    }
  }
  // out of items: from here on this wave's slot is idle (many waves write the same word: harmless)
  if (!final && lane == 0) split_poke(split_flag_addr(split, round), 1u);
}

// The voxels of the suspended packets, from their merged minima.
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) void k_split_finish(GridParams g, const uint32_t* __restrict__ plane, float* __restrict__ out, SplitCtl split, PeerOut peers) {
  constexpr uint32_t AW = MODE == MODE_NORMAL_FOLD ? 128u : 64u;
  const int lane = threadIdx.x & 63;
  const uint32_t n_slots = min(split.cnt[0], split.cap_slots);
  for (uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6); slot < n_slots; slot += gridDim.x * 4u) {
    const uint32_t packet = split.slot_packet[slot];
    if (packet == 0xffffffffu) continue;                                   // walked to the end by its own wave after all
    const GridBrick vox = grid_lane_voxel(g, packet, lane);
    const uint32_t* acc = split.acc + (size_t)slot * AW;
    Best<MODE> best;
    best.d2 = __uint_as_float(acc[lane]);
    if (MODE == MODE_NORMAL_FOLD) best.d2pos = __uint_as_float(acc[64 + lane]);
    bool negate = false;
    if (MODE == MODE_UNSIGNED && SIGN == SIGN_GRID_PLANE) {
      const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
      negate = (plane[w] >> (vox.z & 31u)) & 1u;
    }
    const float result = finish<MODE>(best, negate);
    const size_t out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;
    store_grid_result(out, out_index, result, vox.in_range, g, vox, peers, lane);
  }
}
// Clears the counters and flags of a split walk; `forced`: the flags start raised (every walk is suspended at its first check).
__global__ void k_split_init(uint32_t* __restrict__ cnt, uint32_t forced) {
  for (uint32_t i = threadIdx.x; i < SPLIT_CNT_WORDS; i += blockDim.x) cnt[i] = i >= 16u ? forced : 0u;   // forced: every flag starts raised
}

// The lane walks gather per-lane records; the compiler's own choice (104 VGPRs, 4 waves per SIMD) hides less of that latency than six
// waves with 96 bytes of scratch do: 128^3 x blob-1M 8.9 -> 7.7 ms, 1 M queries 2.75 -> 2.63 ms, the small cases unchanged.
#ifndef M2S_LANE_WAVES
#define M2S_LANE_WAVES 6
#endif
// ---- the lane walk's tree traversal -------------------------------------------------------------------------
// walk_range: the pre-order records [off, limit) of the oriented-bound tree, one lane on its own, at most max_steps node tests.
// ANY slot may start a range: every slot holds a valid record (k_emit / k_node_ext write one per node, the descendants of a
// collapsed leaf included), a range that starts inside a subtree simply meets that subtree's nodes without their ancestors'
// pruning, and every leaf of the range is either met or skipped with a pruned ancestor that lies in the range itself.
template <int MODE>
__device__ __forceinline__ void walk_range(const DeviceMesh& mesh, f3 p, float slack, Best<MODE>& best, float& thr, uint32_t& off,
                                           uint32_t limit, uint32_t max_steps, uint32_t& st_nodes, uint32_t& st_exact) {
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  const char* ext_bytes = reinterpret_cast<const char*>(mesh.ext);
  for (uint32_t s = 0; s < max_steps && off < limit; ++s) {
    const NodeExt nr = *reinterpret_cast<const NodeExt*>(ext_bytes + off);
    ++st_nodes;
    if (ext_dist2(p, nr) > thr) { off = nr.skip; continue; }
    if (nr.tri >= 0) {
      const uint32_t cnt = (nr.skip - off + NB) / (2u * NB);
      for (uint32_t k = 0; k < cnt; ++k) {
        if (!(planes_dist2(p, mesh.planes[nr.tri + k]) > thr)) {
          eval_triangle<MODE>(best, p, mesh.tris[nr.tri + k]);
          thr = prune_bound(best.d2, slack);
          ++st_exact;
        }
      }
      off = nr.skip;
    } else {
      off += NB;
    }
  }
}
// lane_tree_walk: every lane walks the whole tree for its own point — ROUND node tests at a time — and lanes that run out of work
// take over a share of their neighbours'.  A lane near the centre of curvature of a dimple meets hundreds of tied triangles (1 300
// node tests against 160 for the average lane of a 16^3 grid) and a small launch lasts as long as its longest chain of dependent
// loads; the wave as a whole has 64 x 160 tests to do.  After every round the unfinished ranges are published in LDS and ALL lanes
// are dealt out over them again (range k goes to the lanes with lane % K == k, cut into equal pieces): a lane then walks a piece of
// another lane's range for that lane's point, starting from that lane's current bound, and folds what it finds into the owner's
// slot with LDS atomic minima.  Any slot can start a range (walk_range).  Same triangles or more, same arithmetic per triangle:
// bit-identical.
struct LaneShare {
  unsigned long long key[64];   // MODE_NEAREST_NORMAL: (d2 bits, index, !positive): the lexicographic minimum rtree.rs:118-123 asks for
  uint32_t a[64], b[64];        // d2 bits (and d2pos bits for the Normal fold); non-negative floats order like their bit patterns
  uint32_t flag[64];            // Normal fold: a NaN distance was met
  uint32_t rng[64][3];          // unfinished ranges of this round: first, end, owner
  float4 pt[64];                // every lane's point and slack
};
template <int MODE>
__device__ __forceinline__ void lane_tree_walk(const DeviceMesh& mesh, f3 p, float slack, Best<MODE>& best, bool valid,
                                               uint32_t& st_nodes, uint32_t& st_exact, LaneShare& sh) {
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  constexpr uint32_t ROUND = 64;
  const uint32_t end = mesh.n_nodes * NB;
  const uint32_t lane = threadIdx.x & 63u;
  auto key_of = [](const Best<MODE>& x) {
    return ((unsigned long long)__float_as_uint(x.d2) << 32) | ((unsigned long long)(x.idx & 0x7fffffffu) << 1) | (x.pos ? 0ull : 1ull);
  };
  sh.pt[lane] = make_float4(p.x, p.y, p.z, slack);
  sh.a[lane] = __float_as_uint(best.d2);
  sh.b[lane] = __float_as_uint(best.d2pos);
  sh.flag[lane] = best.nan ? 1u : 0u;
  if (MODE == MODE_NEAREST_NORMAL) sh.key[lane] = key_of(best);
  uint32_t owner = lane, off = valid ? 0u : end, limit = end;
  f3 tp = p;
  float tsl = slack;
  Best<MODE> b = best;
  float thr = prune_bound(b.d2, tsl);
  for (;;) {
    walk_range<MODE>(mesh, tp, tsl, b, thr, off, limit, ROUND, st_nodes, st_exact);
    const unsigned long long unf = __ballot(off < limit);
    if (unf == ~0ull) continue;                             // nobody is idle
    // fold what this lane has found into its owner's slot
    if (MODE == MODE_NEAREST_NORMAL) atomicMin(&sh.key[owner], key_of(b));
    else {
      atomicMin(&sh.a[owner], __float_as_uint(b.d2));
      if (MODE == MODE_NORMAL_FOLD) { atomicMin(&sh.b[owner], __float_as_uint(b.d2pos)); if (b.nan) atomicOr(&sh.flag[owner], 1u); }
    }
    if (unf == 0ull) break;
    const uint32_t K = (uint32_t)__popcll(unf);
    if (off < limit) {
      const uint32_t r = (uint32_t)__popcll(unf & ((1ull << lane) - 1ull));
      sh.rng[r][0] = off; sh.rng[r][1] = limit; sh.rng[r][2] = owner;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t k = lane % K, idx = lane / K, helpers = (64u - k + K - 1u) / K;
    const uint32_t so = sh.rng[k][0], se = sh.rng[k][1], sowner = sh.rng[k][2];
    const uint32_t records = (se - so) / NB, piece = (records + helpers - 1u) / helpers;
    off = min(se, so + idx * piece * NB);
    limit = min(se, off + piece * NB);
    owner = sowner;
    const float4 q = sh.pt[owner];
    tp = mk3(q.x, q.y, q.z);
    tsl = q.w;
    // start from the owner's current result: the tightest bound anybody has for that point
    b = Best<MODE>();
    if (MODE == MODE_NEAREST_NORMAL) {
      const unsigned long long kk = sh.key[owner];
      b.d2 = __uint_as_float((uint32_t)(kk >> 32)); b.idx = (uint32_t)(kk >> 1) & 0x7fffffffu; b.pos = (kk & 1ull) == 0ull;
      if (b.idx == 0x7fffffffu) b.idx = 0xffffffffu;        // "none yet" survives the 31-bit trip
    } else {
      b.d2 = __uint_as_float(sh.a[owner]);
      if (MODE == MODE_NORMAL_FOLD) b.d2pos = __uint_as_float(sh.b[owner]);
    }
    thr = prune_bound(b.d2, tsl);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                        // the ranges are read: the next round may overwrite them
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (MODE == MODE_NEAREST_NORMAL) {
    const unsigned long long kk = sh.key[lane];
    best.d2 = __uint_as_float((uint32_t)(kk >> 32)); best.idx = (uint32_t)(kk >> 1) & 0x7fffffffu; best.pos = (kk & 1ull) == 0ull;
  } else {
    best.d2 = __uint_as_float(sh.a[lane]);
    if (MODE == MODE_NORMAL_FOLD) { best.d2pos = __uint_as_float(sh.b[lane]); best.nan = sh.flag[lane] != 0u; }
  }
}

// Per-lane greedy descent (towards the child box nearer to p) and evaluation of the leaf it ends in: a second starting candidate for
// the lane walks.  Their lattice seed is only as good as the lattice is fine — one point per 4^3 voxels of a 16^3 grid is 64 seeds
// for the whole box — and a lane that starts with a loose bound walks long: the launch lasts as long as its slowest lane.
template <int MODE>
__device__ __forceinline__ void greedy_leaf(const DeviceMesh& mesh, f3 p, Best<MODE>& best) {
  uint32_t n = 0;
  NodeRec nr = mesh.nodes[0];
  while (nr.tri < 0) {
    const uint32_t l = n + 1;
    const NodeRec nl = mesh.nodes[l];
    const uint32_t r = nl.skip;
    const NodeRec nrr = mesh.nodes[r];
    const float dl = box_dist2(p, nl.mnx, nl.mny, nl.mnz, nl.mxx, nl.mxy, nl.mxz);
    const float dr = box_dist2(p, nrr.mnx, nrr.mny, nrr.mnz, nrr.mxx, nrr.mxy, nrr.mxz);
    const bool go_left = dl <= dr;
    n = go_left ? l : r;
    nr = go_left ? nl : nrr;
  }
  const uint32_t cnt = (nr.skip - n + 1u) >> 1;
  for (uint32_t k = 0; k < cnt; ++k) eval_triangle<MODE>(best, p, mesh.tris[(uint32_t)nr.tri + k]);
}

// ---- k_lane ---------------------------------------------------------------------------------
// One VOXEL per lane, every lane walking the tree on its own (per-lane offsets, records by vector gathers).
// For the opposite regime of k_packet: when the triangles are much smaller than the voxels (a 1 M-triangle
// scan into a 128^3 grid), the 64 voxels of a brick each need a different handful of triangles; the packet walk
// then runs every exact evaluation wave-wide for the benefit of one lane (blob-1M in 128^3: 11.8 ms), while
// independent walks only pay for what each voxel needs.  Same bounds, same leaf pre-test, same arithmetic, same
// per-brick seed; the result is the exact minimum either way.
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(M2S_LANE_WAVES, 8))) void k_lane(DeviceMesh mesh, GridParams g, const uint32_t* __restrict__ plane,
                                              float* __restrict__ out, int* __restrict__ err, uint32_t n_packets,
                                              const uint32_t* __restrict__ seed_in, uint32_t seed_shift, uint32_t seed_ny, uint32_t seed_nz,
                                              uint32_t bx_off, PeerOut peers) {
  const int lane = threadIdx.x & 63;
  const uint32_t packet = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (packet >= n_packets) return;
  const GridBrick vox = grid_lane_voxel(g, packet, lane);
  if (!vox.brick_in_grid) return;
  const f3 p = grid_point(g, vox);
  const size_t out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;
  const bool LANE_VALID = vox.in_range;                // lanes beyond the grid's edge hold a clamped copy: nothing to walk for them

  Best<MODE> best;
  if (mesh.n_nodes) {
    const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
    uint32_t slot = 0;
    if (seed_in != nullptr)
      slot = min(seed_in[(((vox.bx + bx_off) >> seed_shift) * seed_ny + (vox.by >> seed_shift)) * seed_nz + (vox.bz >> seed_shift)], mesh.n_tris - 1);
    eval_triangle<MODE>(best, p, mesh.tris[slot]);
    greedy_leaf<MODE>(mesh, p, best);
    uint32_t st_nodes = 0, st_exact = 0;               // M2S_STATS
    __shared__ LaneShare lane_share[4];                // one per wave of the workgroup
    lane_tree_walk<MODE>(mesh, p, slack, best, LANE_VALID, st_nodes, st_exact, lane_share[threadIdx.x >> 6]);
    if (mesh.stats != nullptr && LANE_VALID) {         // per lane: the lane walk's unit is the lane
      atomicAdd(&mesh.stats[0], (unsigned long long)st_nodes);
      atomicAdd(&mesh.stats[2], (unsigned long long)st_exact);
      atomicAdd(&mesh.stats[3], 1ull);
      atomicMax(&mesh.stats[72], (unsigned long long)st_nodes);
      atomicMax(&mesh.stats[73], (unsigned long long)st_exact);
    }
  }
  bool negate = false;
  if (MODE == MODE_UNSIGNED && SIGN == SIGN_GRID_PLANE) {
    const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
    negate = (plane[w] >> (vox.z & 31u)) & 1u;                         // grid.rs:630-636
  }
  if (MODE == MODE_NORMAL_FOLD && best.nan) atomicOr(err, ERRF_NAN);
  const float result = finish<MODE>(best, negate);
  if (vox.in_range) {
    out[out_index] = result;
    for (uint32_t i = 0; i < peers.n; ++i) peers.p[i][out_index + (size_t)g.out_off] = result;
  }
}

// ---- k_lane_q: the lane walk for generic queries ---------------------------------------------
// One sorted query per lane, every lane on its own through the tree (as k_lane) and, for the best-of-three-rays sign, through the
// box tree along each axis.  For SPARSE query sets: a packet of 64 of 100 000 queries in the benchmark box is 44 cells of the 512^3
// grid wide, the wave-uniform walk pays for the union of what its lanes need (800 node tests and 340 exact evaluations per packet
// on average, 4 300 and 2 200 for the worst one) and, with fewer packets than the GPU has wave slots, the launch lasts as long as
// that one wave's chain of dependent loads: 3.2 ms for 100 000 queries, 2.7 ms for 1 M.  A lane alone needs ~60 node tests.
template <int AXIS>
__device__ __forceinline__ uint32_t stab_count_lane(const DeviceMesh& mesh, f3 p) {
  uint32_t count = 0, node = 0;
  while (node < mesh.n_nodes) {
    const NodeRec nr = mesh.nodes[node];
    if (!ray_meets_box<AXIS>(p, mk3(nr.mnx, nr.mny, nr.mnz), mk3(nr.mxx, nr.mxy, nr.mxz))) { node = nr.skip; continue; }
    if (nr.tri >= 0) {
      const uint32_t cnt = (nr.skip - node + 1u) >> 1;
      for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t vi = 3u * ((uint32_t)nr.tri + k);
        const float4 c0 = mesh.corners[vi], c1 = mesh.corners[vi + 1u], c2 = mesh.corners[vi + 2u];
        const f3 a = mk3(c0.x, c0.y, c0.z), b = mk3(c0.w, c1.x, c1.y), c = mk3(c1.z, c1.w, c2.x);
        f3 mn, mx;
        triangle_bounding_box(a, b, c, &mn, &mx);     // the candidate rule is per triangle: ITS padded box
        float t;
        const bool h = ray_meets_box<AXIS>(p, mn, mx) && ray_triangle_aligned<AXIS>(p, a, b, c, &t);
        count += h ? 1u : 0u;
      }
      node = nr.skip;
    } else {
      node = node + 1;
    }
  }
  return count;
}
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(M2S_LANE_WAVES, 8))) void k_lane_q(DeviceMesh mesh, const float4* __restrict__ qsorted, const uint32_t* __restrict__ perm,
                                                uint32_t n_q, float* __restrict__ out, int* __restrict__ err,
                                                const uint32_t* __restrict__ seed_in, const GridParams* __restrict__ seed_lattice) {
  const uint32_t i_raw = blockIdx.x * blockDim.x + threadIdx.x;
  const bool LANE_VALID = i_raw < n_q;                 // the last wave's spare lanes stay: the wave-cooperative tail of the walk needs all 64
  const uint32_t i = min(i_raw, n_q - 1u);
  const float4 q = qsorted[i];
  const f3 p = mk3(q.x, q.y, q.z);
  Best<MODE> best;
  if (mesh.n_nodes) {
    const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
    uint32_t slot = 0;
    if (seed_in != nullptr) slot = min(seed_in[query_lattice_cell(*seed_lattice, p.x, p.y, p.z)], mesh.n_tris - 1);
    eval_triangle<MODE>(best, p, mesh.tris[slot]);
    greedy_leaf<MODE>(mesh, p, best);
    uint32_t st_nodes = 0, st_exact = 0;               // M2S_STATS
    __shared__ LaneShare lane_share[4];                // one per wave of the workgroup
    lane_tree_walk<MODE>(mesh, p, slack, best, LANE_VALID, st_nodes, st_exact, lane_share[threadIdx.x >> 6]);
    if (mesh.stats != nullptr && LANE_VALID) {         // per lane: the lane walk's unit is the lane
      atomicAdd(&mesh.stats[0], (unsigned long long)st_nodes);
      atomicAdd(&mesh.stats[2], (unsigned long long)st_exact);
      atomicAdd(&mesh.stats[3], 1ull);
      atomicMax(&mesh.stats[72], (unsigned long long)st_nodes);
      atomicMax(&mesh.stats[73], (unsigned long long)st_exact);
    }
  }
  bool negate = false;
  if (MODE == MODE_UNSIGNED && SIGN == SIGN_RAYS3) {
    const uint32_t cx = stab_count_lane<0>(mesh, p), cy = stab_count_lane<1>(mesh, p);
    uint32_t cz = cx;                                                  // two agreeing parities are the majority (see k_packet)
    if (((cx ^ cy) & 1u) != 0u) cz = stab_count_lane<2>(mesh, p);
    negate = ((cx & 1u) + (cy & 1u) + (cz & 1u)) > 1u;                 // bvh.rs:131-141, rtree_bvh.rs:161-171
  }
  if (!LANE_VALID) return;
  if (MODE == MODE_NORMAL_FOLD && best.nan) atomicOr(err, ERRF_NAN);
  out[perm[i]] = finish<MODE>(best, negate);
}

// ---- host part: which path a call takes (choose_grid_walk), then the launches -------------------------------------------------

// k_packet's parameter list by name.  A call site assigns what it has: the grid path the planes, the seed lattice's shape, the peers and the
// split walk; the query path the sorted queries, their packet table (in `plane`'s place) and the lattice's description.
struct PacketArgs {
  DeviceMesh mesh{};
  GridParams g{};
  const float4* qsorted = nullptr;
  const uint32_t *perm = nullptr, *plane = nullptr;
  uint32_t n_q = 0, n_packets = 0;
  float* out = nullptr;
  int* err = nullptr;
  const uint32_t* seed_in = nullptr;
  uint32_t seed_shift = 0, seed_ny = 0, seed_nz = 0;
  const GridParams* seed_lattice = nullptr;
  CutList cut = {nullptr, 0, 0, 0, 0, nullptr, 0};
  PeerOut peers{};
  SplitCtl split{};
};
// `defer`: the leaf-work form asked for (GridWalkChoice::defer, M2S_DEFER).  Form 2 exists for grids only, and a split walk (grids; a.split.cnt
// set) always queues its evaluations — the follow-up rounds do —: DEFER 3 if asked for, else 1.  `gather_ahead` (M2S_GATHER_AHEAD): the plain
// DEFER 3 walk with its pre-test gathers issued ahead (k_packet's GA form); the split walk and the other forms have no such variant.
// It is taken where it is asked for (1) and, left to the automatic setting (-1), by the forms it was measured to win on: the grid walk of the
// unsigned distance (the headline, configs 2 and 4) and the queries' walk with the three-ray sign (config 3; Bvh(Raycast) and RtreeBvh both run
// it).  The Normal fold and the nearest-with-normal walk keep the plain form until they are measured (profiles/gather_ahead_ab.txt).
// M2S_SEED_SKIP: what the packet kernels OR into their seed's slot (k_packet `seed_none`): 0 — the walk passes over the seed's leaf triangle,
// which the prologue has evaluated for every lane — where the knob says 1 or is left to the automatic setting (-1: every packet form,
// profiles/seed_skip_ab.txt), 0xffffffff ("none": the walk evaluates it again, the same bits) where it says 0.
std::atomic<uint64_t> g_seed_skip_launches{0};   // test hook (m2s_debug_seed_skip_launches): launches whose walks pass over their seed so far
static uint32_t seed_none_word() { return tuning().seed_skip != 0 ? 0u : 0xffffffffu; }
// ... for a launch of a plain k_packet form or of the packet groups (counted: the split forms never pass over it)
static uint32_t seed_none_word_counted() {
  const uint32_t w = seed_none_word();
  if (w == 0u) g_seed_skip_launches.fetch_add(1, std::memory_order_relaxed);
  return w;
}
std::atomic<uint64_t> g_gather_ahead_launches{0};   // test hook (m2s_debug_gather_ahead_launches): launches of a GA form so far
template <bool GRID, int MODE, int SIGN>
void launch_packet(hipStream_t st, const PacketArgs& a, int defer, int gather_ahead_knob) {
  constexpr bool measured = MODE == MODE_UNSIGNED && (GRID || SIGN == SIGN_RAYS3);
  const bool gather_ahead = gather_ahead_knob > 0 || (gather_ahead_knob < 0 && measured);
  const uint32_t per = 8u << XCD_RUN_LOG;                              // one run on each of the eight XCDs
  const uint32_t grid_blocks = ((a.n_packets + per - 1) / per) * per;  // a whole number of runs per XCD (xcd_remap)
  const auto launch = [&](auto stats, auto split, auto form, auto ahead) {
    hipLaunchKernelGGL((k_packet<GRID, MODE, SIGN, decltype(stats)::value, decltype(split)::value, decltype(form)::value, decltype(ahead)::value>), dim3(grid_blocks), dim3(64), 0, st,
                       a.mesh, a.g, a.qsorted, a.perm, a.n_q, a.plane, a.out, a.err, a.n_packets, a.seed_in, a.seed_shift, a.seed_ny, a.seed_nz, a.seed_lattice,
                       a.cut, a.peers, decltype(split)::value ? a.split : plain_ctl(seed_none_word_counted()));
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  constexpr std::integral_constant<int, 0> f0{};
  constexpr std::integral_constant<int, 1> f1{};
  constexpr std::integral_constant<int, 2> f2{};
  constexpr std::integral_constant<int, 3> f3{};
#ifdef M2S_STATS_BUILD
  // M2S_STATS: the counting variant (a few SALU ops more per node); never suspended, so that a packet's counters are whole.  Only the
  // side library libm2s_stats.so (make stats; tools/exp_stats.py loads it through M2S_LIB) carries these instantiations: the product
  // library's code object is seven k_packet variants smaller.
  if (a.mesh.stats != nullptr) return launch(yes, no, f0, no);
#endif
  if constexpr (GRID && MODE != MODE_NEAREST_NORMAL)
    if (a.split.cnt != nullptr) return defer == 3 ? launch(no, yes, f3, no) : launch(no, yes, f1, no);
  if constexpr (GRID)
    if (defer == 2) return launch(no, no, f2, no);
  if (defer == 3 && gather_ahead) {
    g_gather_ahead_launches.fetch_add(1, std::memory_order_relaxed);
    return launch(no, no, f3, yes);
  }
  return defer == 3 ? launch(no, no, f3, no) : defer ? launch(no, no, f1, no) : launch(no, no, f0, no);
}
// The follow-up rounds and the finish of a split grid walk (after launch_packet on the same stream).
template <int MODE, int SIGN>
void launch_split_rounds(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, const uint32_t* plane, float* out, int* err,
                         const SplitCtl& split, const CutList& cut, const PeerOut& peers) {
  // as many single-wave workgroups as two rounds of the chip's wave slots: enough to fill it whatever the items' lengths, few enough
  // that a wave gets several items of a long list
  constexpr unsigned waves = 16384;
  const bool trace = tuning().split_report >= 2;   // debugging aid: which launch faults
  if (trace) { const hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[m2s split] packet launch: %s\n", hipGetErrorString(e)); }
  for (uint32_t r = 1; r <= split.rounds; ++r) {
    hipLaunchKernelGGL((k_split_round<MODE>), dim3(waves), dim3(64), 0, st, mesh, g, split, cut, r, r == split.rounds, err);
    if (trace) { const hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[m2s split] round %u: %s\n", r, hipGetErrorString(e)); }
  }
  hipLaunchKernelGGL((k_split_finish<MODE, SIGN>), dim3(2048), dim3(256), 0, st, g, plane, out, split, peers);
  if (trace) { const hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[m2s split] finish: %s\n", hipGetErrorString(e)); }
}

}  // namespace
uint64_t gather_ahead_launches() { return g_gather_ahead_launches.load(std::memory_order_relaxed); }
uint64_t seed_skip_launches() { return g_seed_skip_launches.load(std::memory_order_relaxed); }
namespace {
uint32_t host_brick_count(const GridParams& g) { return brick_counts(g).padded; }

}  // namespace

// Split walk: accumulator slots for up to SPLIT_CAP_SLOTS suspended packets, lists of SPLIT_ITEMS_PER_SLOT items per slot and round.
// A launch of more packets than SPLIT_MAX_PACKETS is not split at all: it is hundreds of rounds of the chip's wave slots deep, its tail a
// percent or two of it.  Below that every packet has a slot (a suspended packet can always hand over: no path back into the walk).
constexpr uint32_t SPLIT_MAX_PACKETS = 1u << 19, SPLIT_ITEMS_PER_SLOT = 8;
static uint32_t split_cap_slots(size_t packets) { return (uint32_t)std::min<size_t>(std::max<size_t>(packets, 64), SPLIT_MAX_PACKETS); }
// patience, in ordinary packet times: the launch is packets / slots rounds of the chip's 8 192 wave slots deep, the flag goes up
// when all but the last round have been handed out
static uint32_t split_patience_q8(uint32_t packets, const Tuning& tn) {
  const double rounds_before = std::max(1.0, (double)packets / 8192.0 - 1.0);
  return (uint32_t)std::min(65535.0 * 256.0, 256.0 * tn.split_patience / rounds_before);
}

// Which path the walk of the slab [g.xb, g.xe) takes, with every crossover of DESIGN.md §9 — the ONE place where they live.  Pure: no HIP call,
// no arena memory, nothing read but the arguments (tests/test_capi_cpu.py pins the defaults through m2s_debug_grid_walk_choice).  `n_nodes`,
// `leaf_max`, `counting`: the mesh's tree (0 nodes: a one-shot call built the triangle records only), its leaf size and whether it carries
// the M2S_STATS counters.  An interleaved slab (g.chunk_log < 31) switches off the tiny path (grid_is_tiny) and the packet groups and
// constrains the two-level cut lists: see `interleaved` below.
GridWalkChoice choose_grid_walk(const GridParams& g, size_t n_tris, size_t n_nodes, uint32_t leaf_max, bool counting, int algorithm, const Tuning& tn) {
  GridWalkChoice ch;
  if (slab_is_empty(g)) return ch;
  const BrickCounts bc = brick_counts(g);
  const uint32_t packets = bc.padded;
  const bool interleaved = g.chunk_log < 31u;
  // a one-shot call that found its problem tiny built the triangle records only (no tree: n_nodes == 0); a resident mesh decides here, by the
  // smaller (Raycast) limit: it has its tree already
  if ((n_nodes == 0 && n_tris != 0 && algorithm == 0) || grid_is_tiny(g, n_tris, algorithm, true, tn)) {
    ch.path = GridWalkChoice::ALL_PAIRS_SPLIT;
    return ch;
  }
  const bool brute = algorithm == 1;
  ch.seeds = grid_walk_wants_seeds(g, n_tris, algorithm);
  // Walk flavour: bricks that each meet MANY triangles (triangles much smaller than voxels) are better served by
  // independent per-lane walks.  Estimate: triangles per surface brick ~ T / (6 * bricks^(2/3)).
  const int lane_env = tn.lane_walk;   // -1 auto, 0 never, 1 always
  // measured crossover with the work-sharing lane walk (lane / packet walk, whole call, Raycast): blob-11k 32^3 0.77 / 0.86 ms, 48^3
  // 0.80 / 0.71; blob-100k 64^3 1.71 / 2.85, 96^3 2.19 / 2.12; blob-1M 128^3 8.8 / 12.1, 256^3 32.7 / 14.3: the lane walk wins while
  // there are more than ~8 triangles per brick.  (Round 4, with the packets' exact evaluations run densely — DeferQueue — the
  // crossover is ~18: blob-100k 64^3, 24 per brick, 1.60 / 2.04; 80^3, 12.5, 1.79 / 1.67; blob-11k 32^3, 22, 0.73 / 0.67.)  That is the
  // packet walk WITHOUT the split walk (below), whose launch lasts as long as its heaviest packets; where those can be split — the
  // launch must be deeper than the chip's wave slots for that — the packets win beyond 70 triangles per brick (lane walk / packets /
  // packets split, whole call, tools/exp_lane_vs_split.py, profiles/r04_lane_vs_split.txt): blob-100k 88^3 1.99 / 1.61 / 1.14 ms;
  // blob-1M 96^3 (72 per brick) 5.44 / 8.41 / 4.68, 128^3 7.53 / 9.43 / 4.95, 192^3 15.1 / 8.49 / 6.39.
  const double real_bricks = (double)bc.real, grid_bricks = (double)bc.grid;
  const bool split_possible = !brute && n_nodes != 0 && tn.split != 0 && !counting && packets <= SPLIT_MAX_PACKETS;
  // (automatic: a launch at least 1.25 x the chip's 8 192 wave slots deep, padding of the launch order not counted — the patience is measured from the time it takes to hand
  // the packets out, and a launch that is resident at once has none: blob-100k 80^3, 8 000 packets, 2.33 -> 3.77 ms, blob-11k 64^3
  // 0.54 -> 1.46)
  // With the leaf work queued and leaves of 4 - 8 triangles on coarse grids (end of round 4) the walks are two to three times shorter and
  // their tails with them, and the follow-up rounds' ~0.1 ms only pay on large meshes in coarse grids (walk without / with: blob-1M 112^3 2.80 /
  // 2.55 ms, 128^3 2.72 / 2.12, 160^3 2.54 / 2.40, 192^3 3.16 / 3.06, 256^3 4.79 / 4.98; blob-100k 96^3 0.57 / 0.55, 112^3 0.59 / 0.75, 128^3
  // 0.55 / 0.63, 160^3 0.86 / 0.80, 256^3 1.59 / 1.55; the 64-layer slabs of 512^3 x blob-1M 2.44 ... 2.99 / 2.57 ... 2.89): automatic from
  // 300 000 triangles and 5 per brick of the whole grid on.
  const bool split_auto = split_possible && tn.split < 0 && real_bricks >= 10240.0 && n_tris >= 300000u && (double)n_tris >= 5.0 * grid_bricks;
  const double lane_ratio = split_auto ? tn.lane_ratio_split : tn.lane_ratio;
  // (a tree with larger leaves — a one-shot call over a coarse grid, grid_leaf_max — is built for the packets: blob-100k 32^3, 195 triangles per
  // brick, lane walk over leaves of 2 / packets over leaves of 8: 1.68 / 1.67 ms, 48^3 1.74 / 1.18; blob-1M 48^3 5.23 / 4.83, 80^3 5.41 / 4.62)
  const bool lane_walk = !brute && n_tris && (lane_env >= 0 ? lane_env == 1 : (leaf_max <= 2u && (double)n_tris > lane_ratio * real_bricks));
  // cut lists: the top of the tree is walked once per block of 2^log bricks per axis (k_cut)
  // k_cut costs about 0.25 us per brick plus a latency floor of ~0.1 ms; measured crossover (blob-100k / blob-6k,
  // tools/exp_cutmin.py): 192^3 = 110 592 packets loses 0.1-0.2 ms with the lists, 256^3 = 262 144 packets breaks even or
  // gains, 512^3 gains 1.3 ms.  The tests lower it to cover small grids.
  // (asynchronous calls are the pieces of a caller who pipelines them on two streams: k_cut then runs under the previous
  // piece's walk and pays from about half that size)
  const uint32_t cut_min_packets = tn.cut_min_packets;   // 100 000 (round 2: 200 000 for synchronous calls; re-measured with the 64-byte lists: 224^3 2.88 -> 2.75 ms, 192^3 2.41 -> 2.38, 160^3 2.04 -> 2.07)
  if (!brute && !lane_walk && ch.seeds && packets >= cut_min_packets) {
    // two levels (k_cut LEVEL 1 + 2; M2S_CUT_COARSE: -1 automatic, 0 never, 1 always).  The coarse launch is waves / 8 waves of its own whose longest
    // chain (the subtree next to its region, up to the visit cap) is ~0.14 ms whatever the grid: 1024^3 (262 144 fine waves) seed + cut 5.98 -> 4.9 ms and
    // the call 83.2 -> 81.9 ms (sheet-100k, Normal) / 40.8 -> 39.9 (blob-100k); 512^3 (32 768) 0.72 -> 0.67 + 0.14 ms with a walk 0.08 ms shorter — a wash;
    // a 64-layer slab of 512^3 (4 096) 0.20 -> 0.34 ms.  Automatic from M2S_CUT_COARSE_MIN_WAVES = 40 000 fine waves on (profiles/r06_cut_coarse.txt; the
    // tests force it on small grids).  A block must lie inside one chunk of an interleaved slab.  (The seed lattice has one point per brick — shift 0
    // —, which the coarse level relies on.)
    const int cc = tn.cut_coarse;
    const size_t waves = cut_blocks(g, 2);   // blocks of 4 x 4 x 4 bricks = fine waves
    const bool blocks_ok = !interleaved || g.chunk_log >= g.bl[0] + 2u;
    const bool two_level = blocks_ok && (cc > 0 || (cc < 0 && waves >= tn.cut_coarse_min_waves));
    ch.cut_levels = two_level ? 2 : 1;
  }
  // packet groups (k_packet_group; M2S_GROUP: -1 automatic, 0 never, 1 always): launches of at most M2S_GROUP_MAX_PACKETS packets without
  // cut lists where the bricks meet several triangles each (the chains are long there: 64^3 ... 128^3 over 100 k triangles)
  const int gk = tn.group;
  // (not where the split walk is the automatic choice — large meshes in launches deeper than the chip: blob-1M 96^3 Raycast 1.88 ms split, 2.48 in groups)
  const bool can = !brute && !lane_walk && ch.cut_levels == 0 && n_nodes != 0 && !counting && tn.split <= 0 && !split_auto && tn.defer < 0 && !interleaved;
  const bool want = gk > 0 || (gk < 0 && (double)n_tris >= tn.group_min_ratio * real_bricks);
  if (can && want) {
    // as many waves per packet (a power of two, four at most) as keep the launch within M2S_GROUP_TARGET_WAVES waves
    uint32_t w = 1;
    while (w < GROUP_MAX_WAVES && (double)(2u * w) * real_bricks <= (double)tn.group_target_waves) w *= 2;
    if (gk > 0 && w < 2u) w = GROUP_MAX_WAVES;                      // forced (tests)
    if (w >= 2u) ch.group_waves = w;
  }
  // split walk (packet walk only; M2S_SPLIT: -1 / 1 on, 0 off, 2 on with the flags raised from the start)
  // Where it pays (tools/exp_split.py, exp_split_rank.py; walk with / without): the stragglers are the packets deep inside a body
  // whose voxels see many triangles at (nearly) the same distance, and they weigh the more the finer the mesh is against the grid —
  // blob-100k in 96^3 ... 192^3 1.79 -> 1.07, 1.57 -> 1.28, 1.81 -> 1.63 ms, in 256^3 2.25 -> 2.34 (a wash), the 64-layer slabs of
  // 512^3 1.21 -> 1.26 (a loss: no tail to speak of, three more launches); blob-1M in 256^3 12.8 -> 9.5 ms, its slowest 8-GPU slab of
  // 512^3 5.05 -> 4.05, its fastest 3.14 -> 3.16.  Automatic: split_auto above (>= 300 000 triangles, >= 5 per packet brick of the WHOLE grid, >= 10 240 bricks).
  ch.split = !lane_walk && split_possible && ch.group_waves == 0 && (tn.split > 0 || split_auto);
  ch.split_forced = ch.split && tn.split == 2;
  // The packet walk's leaf work (DeferQueue; M2S_DEFER forces a form): 0 wave-wide at once, 1 the exact evaluations queued per (voxel, triangle) pair,
  // 2: queued, but at once where most of the wave is reached (grids much finer than the mesh: see DEFER_DIRECT_LANES),
  // 3: the pre-tests queued too (defer_pretest) — from 0.045 triangles per brick on: walk, queued evaluations / + queued pre-tests, blob-100k
  // 128^3 1.02 / 0.83 ms, 256^3 1.74 / 1.48, 512^3 (0.048 per brick) 6.85 / 6.54, 768^3 (0.014) 16.9 / 17.7; blob-1M 512^3 21.9 / 18.2; blob-11k
  // 256^3 (0.04) 0.60 / 0.63; sheet-100k 512^3 (0.05) 13.2 / 12.0.  (Both forms of pre-test in one kernel, chosen per leaf by the number of lanes that
  // want it, cost the dense regime what they gained the sparse one: 128^3 0.83 -> 0.92, 768^3 17.7 -> 16.9.)
  ch.defer = tn.defer == 0 ? 0 : tn.defer > 0 ? tn.defer : ((double)n_tris < 0.02 * grid_bricks ? 2 : (double)n_tris < 0.045 * grid_bricks ? 1 : 3);
  ch.gather_ahead = tn.gather_ahead;   // (which forms the automatic setting takes: launch_packet)
  ch.path = lane_walk ? GridWalkChoice::LANE : ch.group_waves ? GridWalkChoice::GROUP : brute ? GridWalkChoice::ALL_PAIRS : GridWalkChoice::PACKET;
  return ch;
}
// What a call knows before its mesh exists (it sizes its workspace block then): the most permissive mesh — a tree, leaves too large for the lane
// walk, no counters.  Whatever choose_grid_walk splits for a real mesh over (g, n_tris), this splits too (tests/test_capi_cpu.py sweeps it).
GridWalkChoice choose_grid_walk_for_sizing(const GridParams& g, size_t n_tris) { return choose_grid_walk(g, n_tris, 1, ~0u, false, 0, tuning()); }

// Nothing where the split walk cannot run (it was ~235 MB of every 256^3 call's block, ~370 MB from 2^19 packets on), the item lists by the
// rounds in use.
static size_t split_workspace_bytes(const GridParams& g, size_t n_tris, size_t packets) {
  if (!choose_grid_walk_for_sizing(g, n_tris).split) return 0;
  const size_t cap = split_cap_slots(packets);
  const size_t items = std::max<size_t>(cap, std::min<size_t>(cap * SPLIT_ITEMS_PER_SLOT, 1u << 20));
  const size_t rounds = std::min(tuning().split_rounds, SPLIT_MAX_ROUNDS);
  return 256 + SPLIT_CNT_WORDS * 4 + cap * 4 + 256 + cap * 128 * 4 + 256 + rounds * items * 16 + 256;
}
size_t grid_distance_workspace_bytes(const GridParams& g, size_t n_tris) {
  const BrickCounts bc = brick_counts(g);
  const size_t bricks = (size_t)bc.padded;
  if ((double)(g.xe - g.xb) * g.n[1] * g.n[2] <= 4194304.0)   // room for k_brute_split's per-voxel words
    return bricks * 44 + bricks + 16384 + cut_blocks(g, 0) * CUT_WORDS * 4 + cut_blocks(g, 2) * CUTC_S * CUTC_WORDS * 4 + 512 + TOP_SUBTREES * 8 + 256 + bricks * 64 * 8 + 4096 + split_workspace_bytes(g, n_tris, bricks);
  const size_t trail_counters = (size_t)bc.nb[0] * (bc.nb[1] + 1) * 4;   // M2S_PEER_TRAIL progress
  return bricks * 44 + bricks + 16384 + cut_blocks(g, 0) * CUT_WORDS * 4 + cut_blocks(g, 2) * CUTC_S * CUTC_WORDS * 4 + 512 + TOP_SUBTREES * 8 + 256 + trail_counters + 1024 + split_workspace_bytes(g, n_tris, bricks);   // seeds + cut lists (one per brick) + split walk
}

uint32_t host_packet_bricks(const GridParams& g) { return slab_is_empty(g) ? 0u : host_brick_count(g); }
bool grid_walk_wants_seeds(const GridParams& g, size_t n_tris, int algorithm) { return algorithm != 1 && n_tris && host_packet_bricks(g) >= 8; }

// Seeds and cut lists for the slab [g.xb, g.xe) (everything a walk needs besides the mesh) — what choose_grid_walk says the walk takes;
// `launch_grid_walk` then walks the slab, or any x-piece of it that starts on a block boundary.  `raw_seeds` (optional): a seed lattice
// computed from the input-order centroids while the mesh was being built; its ids are translated to sorted slots here.
int prepare_grid_walk(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const GridParams& g, int algorithm, bool pipelined,
                      GridWalkPlan* plan, const SeedLattice* raw_seeds) {
  *plan = GridWalkPlan{};
  const Tuning& tn = tuning();
  const GridWalkChoice ch = choose_grid_walk(g, mesh.n_tris, mesh.n_nodes, mesh.leaf_max, mesh.stats != nullptr, algorithm, tn);
  plan->choice = ch;
  if (ch.path == GridWalkChoice::NOTHING) return 0;
  M2S_REQUIRE_GRID_CONSTS(g);
  const BrickCounts bc = brick_counts(g);
  const uint32_t packets = bc.padded;
  if (ch.path == GridWalkChoice::ALL_PAIRS_SPLIT) {
    plan->brute_acc = ws.take<uint32_t>((size_t)packets * 64 * 2);
    if (!plan->brute_acc) { set_error("internal: brute-force workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    return 0;
  }
  if (ch.seeds) {
    SeedLattice lat;
    if (raw_seeds && raw_seeds->ids) {
      lat = *raw_seeds;
      launch_seed_remap(st, lat.ids, lat.points, mesh.slot_of, mesh.n_tris);
    } else {
      const int rc = launch_grid_seeds(ws, st, mesh.cen, mesh.n_tris, g, &lat);
      if (rc) return rc;
    }
    plan->seeds = lat.ids; plan->seed_shift = lat.shift; plan->seed_ny = lat.ny; plan->seed_nz = lat.nz;
  }
  if (ch.cut_levels) {   // the top of the tree is walked once per block of 4 x 4 x 4 bricks (k_cut), in one level or two
    uint32_t* lists = ws.take<uint32_t>((size_t)bc.real * CUT_WORDS);
    if (!lists) { set_error("internal: cut-list workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    uint32_t* coarse = nullptr;
    if (ch.cut_levels == 2) {
      coarse = ws.take<uint32_t>(cut_blocks(g, 2) * CUTC_S * CUTC_WORDS);   // blocks of 4 x 4 x 4 bricks = fine waves
      if (!coarse) { set_error("internal: cut-list workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    }
    launch_grid_cut(st, mesh, g, plan->seeds, plan->seed_shift, plan->seed_ny, plan->seed_nz, lists, coarse);
    plan->cut_lists = lists; plan->cut_log = 0; plan->cut_ny = bc.nb[1]; plan->cut_nz = bc.nb[2]; plan->cut_coarse = coarse;
    plan->cut_words = (size_t)bc.real * CUT_WORDS; plan->cut_coarse_words = coarse ? cut_blocks(g, 2) * CUTC_S * CUTC_WORDS : 0;
  }
  if (ch.path == GridWalkChoice::GROUP) {
    uint2* top = ws.take<uint2>(TOP_SUBTREES);
    if (!top) { set_error("internal: workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    hipLaunchKernelGGL(k_tree_top, dim3(1), dim3(TOP_SUBTREES), 0, st, mesh, top);
    plan->group_top = top;
  }
  if (ch.split) {
    SplitCtl sc;
    sc.cap_slots = split_cap_slots(packets);
    sc.cap_items = std::max(sc.cap_slots, std::min(sc.cap_slots * SPLIT_ITEMS_PER_SLOT, 1u << 20));
    sc.rounds = std::min(tn.split_rounds, SPLIT_MAX_ROUNDS);
    sc.emit_min = std::max(2u, tn.split_min_records) * (uint32_t)sizeof(NodeExt);
    sc.emit_max = std::max(std::max(2u, tn.split_min_records), tn.split_max_records) * (uint32_t)sizeof(NodeExt);
    sc.grace = tn.split_budget ? tn.split_budget : 128u;
    sc.idle_below = ch.split_forced ? 1u : 0u;                             // forced (tests): every stamp is time 0 — all flags up, no patience
    sc.patience_q8 = split_patience_q8(packets, tn);
    sc.cnt = ws.take<uint32_t>(SPLIT_CNT_WORDS);
    sc.slot_packet = ws.take<uint32_t>(sc.cap_slots);
    sc.acc = ws.take<uint32_t>((size_t)sc.cap_slots * 128);
    sc.items = ws.take<uint4>((size_t)sc.rounds * sc.cap_items);
    if (!sc.cnt || !sc.slot_packet || !sc.acc || !sc.items) { set_error("internal: split-walk workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    plan->split = sc;
  }
  return 0;
}

int launch_grid_walk(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, int mode, const uint32_t* d_inside_plane,
                     const GridWalkPlan& plan, uint32_t bx_off, float* d_out, int* d_err, const PeerOut* peers) {
  const GridWalkChoice& ch = plan.choice;
  if (slab_is_empty(g) || ch.path == GridWalkChoice::NOTHING) return 0;
  PeerOut pz{};
  if (peers) pz = *peers;
  const BrickCounts bc = brick_counts(g);
  const uint32_t packets = bc.padded, real = (uint32_t)bc.real;   // (no super-brick padding for k_brute_split)
  const uint32_t* plane = mode == MODE_UNSIGNED ? d_inside_plane : nullptr;   // the Normal fold carries its own sign
  const CutList cut = cut_list_for(mesh.n_nodes, plan.cut_lists, plan.cut_log, plan.cut_ny, plan.cut_nz, bx_off, nullptr);
  M2S_REQUIRE_GRID_CONSTS(g);
  if (ch.path == GridWalkChoice::ALL_PAIRS_SPLIT) {
    M2S_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)plan.brute_acc, 0x7f800000, (size_t)packets * 64 * 2, st));   // +inf: where every search starts (Best<>)
    return launch_grid_brute_split(st, mesh, g, mode, plane, plan.brute_acc, real, d_out, d_err, pz);
  }
  if (ch.path == GridWalkChoice::ALL_PAIRS) return launch_grid_brute(st, mesh, g, mode, plane, d_out, d_err, packets, pz);
  // (the Normal fold's split variants — k_packet<GRID, NORMAL_FOLD, ..., SPLIT, {1, 3}>, k_split_round<NORMAL_FOLD> — need 9 - 11 registers
  // more than eight waves per SIMD leave and spill them to scratch, the very thing that costs this kernel 10 - 40 %: the automatic choice
  // leaves the Normal sign to the plain walk; M2S_SPLIT=1 / 2 still runs them — the tests do)
  const bool split = ch.path == GridWalkChoice::PACKET && ch.split && (mode != MODE_NORMAL_FOLD || tuning().split > 0);
  PacketArgs a;
  a.mesh = mesh; a.g = g; a.plane = plane; a.out = d_out; a.err = d_err; a.n_packets = packets;
  a.seed_in = plan.seeds; a.seed_shift = plan.seed_shift; a.seed_ny = plan.seed_ny; a.seed_nz = plan.seed_nz; a.cut = cut; a.peers = pz;
  if (split) {
    a.split = plan.split;
    // the patience is measured in hand-out rounds of THIS launch (an x-piece of the slab is shallower than the slab the plan was made for)
    if (!ch.split_forced) a.split.patience_q8 = split_patience_q8(packets, tuning());
    hipLaunchKernelGGL(k_split_init, dim3(1), dim3(64), 0, st, a.split.cnt, ch.split_forced ? 1u : 0u);
  }
  for_grid_form(mode, plane != nullptr, [&](auto form) {
    constexpr int MODE = decltype(form)::MODE, SIGN = decltype(form)::SIGN;
    switch (ch.path) {
      case GridWalkChoice::NOTHING: case GridWalkChoice::ALL_PAIRS_SPLIT: case GridWalkChoice::ALL_PAIRS: break;   // (brute.hip: launched above)
      case GridWalkChoice::LANE:
        hipLaunchKernelGGL((k_lane<MODE, SIGN>), dim3((packets + 3) / 4), dim3(256), 0, st, mesh, g, plane, d_out, d_err, packets, a.seed_in, a.seed_shift, a.seed_ny, a.seed_nz, bx_off, pz);
        break;
      case GridWalkChoice::GROUP: {
        const uint32_t per = 8u << XCD_RUN_LOG, grid_blocks = ((packets + per - 1) / per) * per;        // as launch_packet: whole runs per XCD (xcd_remap)
        const size_t lds = ((size_t)ch.group_waves * 256u + DeferLayout<MODE>::SLOT_WORDS) * 4u;
        hipLaunchKernelGGL((k_packet_group<MODE, SIGN>), dim3(grid_blocks), dim3(64 * ch.group_waves), lds, st, mesh, g, plane, d_out, d_err, packets,
                           a.seed_in, a.seed_shift, a.seed_ny, a.seed_nz, bx_off, plan.group_top, pz, seed_none_word_counted());
        break;
      }
      case GridWalkChoice::PACKET:
        launch_packet<true, MODE, SIGN>(st, a, ch.defer, ch.gather_ahead);
        if (split) launch_split_rounds<MODE, SIGN>(st, mesh, g, plane, d_out, d_err, a.split, cut, pz);
        break;
    }
  });
  M2S_HIP_CHECK(hipGetLastError());
  if (split && tuning().split_report) {
    const SplitCtl& sc = a.split;
    uint32_t h[SPLIT_CNT_WORDS];
    M2S_HIP_CHECK(hipStreamSynchronize(st));
    M2S_HIP_CHECK(hipMemcpy(h, sc.cnt, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "[m2s split] %u packets: %u suspended (room for %u); items per round:", packets, h[0], sc.cap_slots);
    for (uint32_t r = 1; r <= sc.rounds; ++r) fprintf(stderr, " %u", h[1 + r]);
    fprintf(stderr, " (room for %u each, reserved in blocks of 64); first look after %u units, patience %.2f of the time to the flag, subtrees of %u .. %u records; XCD 0: handed out in %.1f us\n",
            sc.cap_items, sc.grace, sc.patience_q8 / 256.0, sc.emit_min / (uint32_t)sizeof(NodeExt), sc.emit_max / (uint32_t)sizeof(NodeExt),
            h[16] ? ((h[16] & ~1u) - h[24]) * 0.01 : 0.0);
  }
  return 0;
}

int launch_grid_distance(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const GridParams& g, int mode,
                         const uint32_t* d_inside_plane, int algorithm, float* d_out, int* d_err,
                         hipEvent_t ev_before_final, hipEvent_t wait_before_final, bool pipelined,
                         const SeedLattice* raw_seeds, hipEvent_t wait_raw_seeds, const PeerOut* peers) {
  GridWalkPlan plan;
  if (raw_seeds && wait_raw_seeds) M2S_HIP_CHECK(hipStreamWaitEvent(st, wait_raw_seeds, 0));   // computed on another stream
  int rc = prepare_grid_walk(ws, st, mesh, g, algorithm, pipelined, &plan, raw_seeds);
  if (rc) return rc;
  // the sign planes may have been built beside the seed passes, on another stream (capi.hip): the walk needs them
  if (wait_before_final) M2S_HIP_CHECK(hipStreamWaitEvent(st, wait_before_final, 0));
  if (ev_before_final) M2S_HIP_CHECK(hipEventRecord(ev_before_final, st));
  return launch_grid_walk(st, mesh, g, mode, d_inside_plane, plan, 0, d_out, d_err, peers);
}

// Sparse query sets take the lane walk (k_lane_q): fewer than M2S_QUERY_LANE_COEFF (2.5) queries per triangle.
bool query_walk_is_lane(size_t n_q, size_t n_tris, int sign_src) {
  const int lane_env = tuning().lane_walk;   // -1 auto, 0 never, 1 always
  return n_tris && sign_src != SIGN_XRAY_ALL && (lane_env >= 0 ? lane_env == 1 : (double)n_q < tuning().query_lane_coeff * (double)n_tris);
}
// The leaf size a query call wants (M2S_LEAF_MAX overrides): 2 for the lane walk (every lane pays for its own leaf), for the packets by
// queries per triangle — packets of few queries per triangle are large against the triangles, as bricks of a coarse grid are (packets, leaves of
// 2 / 4 / 8, RtreeBvh, whole call, tools/exp_query_walks.py): blob-100k 1 M queries 1.91 / 1.56 / 1.39 ms, 3 M 2.37 / 2.02 / 1.91, 10 M 3.93 / 3.60 / 3.74;
// blob-11k 300 k 0.66 / 0.63 / 0.63, 3 M 1.00 / 0.95 / 1.04, 10 M 2.19 / 2.30 / 2.77.
uint32_t query_leaf_max(size_t n_q, size_t n_tris, int sign_src) {
  const Tuning& tn = tuning();
  if (tn.leaf_max != 0) return tn.leaf_max;
  if (n_tris == 0 || query_walk_is_lane(n_q, n_tris, sign_src)) return 2u;
  const double per_tri = (double)n_q / (double)n_tris;
  return per_tri < 50.0 ? 8u : per_tri < 500.0 ? 4u : 2u;
}

// The leaf size of a one-shot grid call's tree (M2S_LEAF_MAX overrides).  A larger leaf trades node tests for leaf pre-tests; with
// those queued per (voxel, triangle) pair the optimum moved up wherever a brick meets more than a triangle or so (walk, leaves of 2 / 4 /
// 8, tools/exp_lane_vs_split.py with M2S_LEAF_MAX): blob-100k 64^3 (24 triangles per brick) 1.15 / 0.79 / 0.59 ms, 96^3 (7.2, split) 0.69 /
// 0.57 / 0.54, 128^3 (3.05) 0.87 / 0.74 / -; blob-1M 128^3 (30, split) 2.89 / 2.33 / 2.11, 256^3 (3.8) 6.10 / 5.22 / -; blob-11k 64^3 (2.7) 0.25 /
// 0.21 / 0.20, 96^3 (0.8) 0.22 / 0.20 / 0.21; blob-100k 256^3 (0.38) 1.55 / 1.52 / -, 512^3 (0.048) 6.48 / 7.88 / -.  A persistent mesh's tree is
// re-marked by the grid call that wants another size (set_leaf_size).
uint32_t grid_leaf_max(const GridParams& g, size_t n_tris) {
  const Tuning& tn = tuning();
  if (tn.leaf_max != 0) return tn.leaf_max;
  const double per_brick = (double)n_tris / std::max(1.0, (double)brick_counts(g).grid);
  return per_brick >= 40.0 ? 16u : per_brick >= 3.0 ? 8u : per_brick >= 0.6 ? 4u : 2u;   // (16: blob-100k 32^3, 195 per brick, 1.31 -> 1.11 ms; blob-1M 80^3 3.14 -> 2.53)
}

int prepare_query_lists(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const QueryPlan& plan, const QuerySeeds* pre, const uint32_t** seeds_out,
                        const GridParams** d_lat_out, const uint32_t** lists_out, size_t* list_words) {
  *seeds_out = nullptr; *d_lat_out = nullptr; *lists_out = nullptr;
  if (list_words) *list_words = 0;
  // seeds: jump flooding over a QL^3 lattice on the query bounding box (as for the grid path) — here, or beside the build (`pre`)
  const uint32_t* seeds = nullptr;
  const GridParams* d_lat = nullptr;
  if (plan.seeds && mesh.n_tris) {
    QuerySeeds own;
    if (pre == nullptr || pre->ids == nullptr) {
      const int rc = launch_query_seeds(ws, st, mesh.cen, mesh.n_tris, plan, false, &own);
      if (rc) return rc;
      pre = &own;
    } else if (pre->raw) {
      launch_seed_remap(st, pre->ids, (size_t)QL * QL * QL, mesh.slot_of, mesh.n_tris);
    }
    seeds = pre->ids;
    d_lat = plan.lat;
  }
  if (plan.centres != nullptr && seeds != nullptr) {
    uint32_t* lists = ws.take<uint32_t>((size_t)plan.launched * CUT_WORDS);
    if (!lists) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    launch_query_cut(st, mesh, seeds, plan.launched, lists, plan.centres, plan.table, d_lat);
    *lists_out = lists;
    if (list_words) *list_words = (size_t)plan.launched * CUT_WORDS;
  }
  *seeds_out = seeds; *d_lat_out = d_lat;
  return 0;
}

int launch_query_walk(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const float* d_queries, const QueryPlan& plan,
                      int mode, int sign_src, int algorithm, float* d_out, int* d_err, const QuerySeeds* pre) {
  const size_t n_q = plan.n_q;
  if (n_q == 0) return 0;
  GridParams g{};
  const uint32_t nq = (uint32_t)n_q;
  if (algorithm == 1) return launch_query_brute(st, mesh, d_queries, nq, mode, sign_src, d_out, d_err);
  const uint32_t launched = plan.launched;
  const uint32_t *seeds = nullptr, *lists = nullptr;
  const GridParams* d_lat = nullptr;
  const int rc = prepare_query_lists(ws, st, mesh, plan, pre, &seeds, &d_lat, &lists);
  if (rc) return rc;
  CutList cut = {nullptr, 0, 0, 0, 0, nullptr, 0};
  if (lists != nullptr) cut = cut_list_for(mesh.n_nodes, lists, 0, 0, 0, 0, plan.centres);
  PacketArgs a;
  a.mesh = mesh; a.g = g; a.qsorted = plan.sorted; a.perm = plan.perm; a.n_q = nq; a.plane = plan.table; a.out = d_out; a.err = d_err; a.n_packets = launched;
  a.seed_in = seeds; a.seed_lattice = d_lat; a.cut = cut;
  const int defer = tuning().defer == 0 ? 0 : tuning().defer == 1 ? 1 : 3;
  for_query_form(mode, sign_src, [&](auto form) {
    constexpr int MODE = decltype(form)::MODE, SIGN = decltype(form)::SIGN;
    if (plan.lane_walk) hipLaunchKernelGGL((k_lane_q<MODE, SIGN>), dim3((nq + 255u) / 256u), dim3(256), 0, st, mesh, a.qsorted, a.perm, nq, d_out, d_err, seeds, d_lat);
    else launch_packet<false, MODE, SIGN>(st, a, defer, tuning().gather_ahead);
  });
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_query_distance(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const float* d_queries, size_t n_q,
                          int mode, int sign_src, int algorithm, float* d_out, int* d_err) {
  if (query_is_tiny(n_q, mesh.n_tris, algorithm, sign_src) && mesh.stats == nullptr)
    return launch_query_brute_split(ws, st, mesh, d_queries, n_q, mode, sign_src, d_out, d_err);
  QueryPlan plan;
  const int rc = prepare_query_walk(ws, st, d_queries, n_q, mesh.n_tris, sign_src, algorithm, &plan, nullptr);
  if (rc) return rc;
  return launch_query_walk(ws, st, mesh, d_queries, plan, mode, sign_src, algorithm, d_out, d_err, nullptr);
}

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_distance() {}
void warm_distance(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_distance, dim3(1), dim3(64), 0, st);
  // ... and resolves a kernel FUNCTION at its own first launch (~0.3 ms each): ask for the attributes of the ones a first call uses
  const void* fns[] = {
      (const void*)k_packet<true, MODE_UNSIGNED, SIGN_GRID_PLANE, false, false, 3, true>,   // (the GA forms: what launch_packet takes automatically)
      (const void*)k_packet<true, MODE_UNSIGNED, SIGN_GRID_PLANE, false, false, 2>,
      (const void*)k_packet<true, MODE_NORMAL_FOLD, SIGN_NONE, false, false, 3>,
      (const void*)k_packet<true, MODE_NORMAL_FOLD, SIGN_NONE, false, false, 2>,
      (const void*)k_packet<false, MODE_UNSIGNED, SIGN_RAYS3, false, false, 3, true>,
      (const void*)k_packet<false, MODE_NEAREST_NORMAL, SIGN_NONE, false, false, 3>,
      (const void*)k_split_init,
      (const void*)k_split_round<MODE_UNSIGNED>,
      (const void*)k_split_round<MODE_NORMAL_FOLD>,
      (const void*)k_split_finish<MODE_UNSIGNED, SIGN_GRID_PLANE>,
      (const void*)k_split_finish<MODE_NORMAL_FOLD, SIGN_NONE>,
      (const void*)k_lane<MODE_UNSIGNED, SIGN_GRID_PLANE>,
      (const void*)k_lane_q<MODE_UNSIGNED, SIGN_RAYS3>};
  hipFuncAttributes attr;
  for (const void* f : fns) (void)hipFuncGetAttributes(&attr, f);
  (void)hipGetLastError();
}

}  // namespace m2s
