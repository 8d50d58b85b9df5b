// mbots_kernels.hpp -- device state descriptors and kernel launchers.
#pragma once

#include "mbots_device.hpp"
#include "mbots_traj.hpp"
#include "mbots_render.hpp"
#include "mbots_policy.hpp"
#include "../../include/mbots.h"

namespace mbots {

constexpr uint32_t kFlagRewardFixed = 0x1u;   // MBOTS_FLAG_REWARD_FIXED
constexpr uint32_t kFlagFixDepth = 0x2u;      // MBOTS_FLAG_FIX_DEPTH_ALIAS
constexpr uint32_t kFlagShardGhost = 0x4u;    // MBOTS_FLAG_SHARD_GHOST

// Agent / world state in HBM (SoA).  Agent columns are [W][cap].
struct SimState {
    float *x, *y, *rw, *rz;         // base::Position.xy, base::Rotation (w, z)
    int32_t *species;               // Species
    int32_t *health;                // Health (== HealthAccumulator between steps)
    int32_t *finder;                // FinderOutput hit -> slot in the same world, -1 none
    int32_t *obsrow;                // AgentObservationBridge -> export row (K3a writes it, the
                                    // next K1 reads it)
    float *sur0, *sur1;             // SurroundingObservation (step-local)
    uint32_t *stats;                // AgentStats bits (step-local)
    int32_t *n;                     // [W] live agents per world
    uint32_t *ctr;                  // [W] RNG counter
    uint2 *key;                     // [W] RNG key
    uint64_t *food;                 // [W][48] per chunk: 5 x (x | y << 4) bytes, live mask << 40
    uint32_t *food_rot;             // [W][5][48] food box rotation (22-bit quarter turn) per package
    int32_t *cur_food;              // [W] Sim::currentNumFood
    float *sreward;                 // [W][4] SpeciesReward
    int32_t *scount;                // [W][4] SpeciesCount (exported)
    int32_t *row_base;              // [W][4] first export row of (world, species)
    int32_t *world_off;             // [W] world-major agent offsets
    int32_t *src_of;                // [W*cap] new export row -> old row (-1: new agent)
    // lazy HiddenState (set by the host per step): K3a also stores the row map
    // composed over the stretch, map_out[new] = map_in[old] (map_in null: old;
    // old < 0: -1) -- two buffers by step parity, never the same one
    const int32_t *map_in;
    int32_t *map_out;
    uint32_t *overflow;             // [W] dropped births/respawns
    uint32_t *totals;               // [0] = N, [1..4] = per-species rows, [kTotRows] = table rows
                                    // incl. the shard ghost's (after row N), [kTotOverflow]
    uint32_t *totals_host;          // mapped pinned mirror of totals (written by K2)
    int32_t *tiles;                 // [2][5][ntiles][kTileBuckets] per-tile species/agent counts (K1 -> K2)
    unsigned long long *agent_steps;
    float4 *raytab;                 // [36] per ray (32 pixels, the finder): u, NearPt c, s, e
    int32_t *sorder;                // [W] the sensor's world order (K2: each tile by descending
                                    // population), or null: world order (W not a multiple of
                                    // the 1024-world tile)
    // K1's output half of the double-buffered columns the sensor reads (the
    // sensor of step t runs beside step t+1's K1; swap_state after each K1)
    float *x_out, *y_out, *rw_out, *rz_out;
    int32_t *species_out, *n_out;
    int32_t *obsrow_out;            // K1 -> K3a / the sensor: each slot's old export row (not
                                    // swapped with obsrow -- K1 reads obsrow, K3a rewrites it --
                                    // but one of two buffers by step parity, set by the host:
                                    // in K1-finder mode the sensor of step t reads it beside
                                    // step t+1's K1)
    uint64_t *food_out;
    // the fork as a value wait (small world counts, mbots_step): K2's last
    // block stores `epoch` into sig_fork (signal memory); epoch 0: no flag
    uint32_t *fork_ctr;             // K2 blocks done (reset by the last)
    uint32_t *sig_fork;
    uint32_t epoch;
    uint32_t W, cap, A, world_offset, flags, seed, ntiles;
    // K1 computes the finder slots its actions read itself (world_finders;
    // small world counts) instead of reading the last sensor's S.finder, so it
    // does not wait for that sensor
    uint32_t k1_finder;
    // ... except on the first step after init (no sensor has run: the finder
    // slots are the init's "none", S.finder), set by the host for that launch
    uint32_t finder_from_state;
    // (K1-finder mode) the last table's sensor rows: the sensor itself moves
    // them into its rows' prev-sensor columns (null: the shift / moves do)
    const int8_t *psem_src;
    const uint8_t *pdepth_src;
    uint32_t Wx;                    // exported worlds: W, or W - 1 with the shard ghost (the
                                    // last world, its rows placed after every exported row)
    // mixed capacity classes (agent_capacity > 128 outside K1-finder mode): the
    // 128-slot kernels take every world that fits them and the class kernels
    // only the worlds K2 listed -- big_k1: 2 n + A > 128 (the next K1 could
    // overflow 128 slots), big_s: n > 128 (this step's sensor) -- each [2][W]
    // by step parity, with their counts in big_cnt[parity][2]
    uint32_t mixed;
    uint32_t track_maxpop;          // K2 publishes each tile's largest world (kTotMaxPop; set by
                                    // the first mbots_max_population)
    uint32_t list_par;              // the parity whose lists this launch reads (host-set)
    int32_t *big_k1, *big_s;
    uint32_t *big_cnt;
    // the owed columns' row counts (set by the host per step, or null): K2 stores
    // the table's rows (totals[kTotRows]) into rows_out[0] (lazy HiddenState)
    // and rows_out[2] (owed PrevAction) -- words by step parity, two apart
    uint32_t *rows_out;
};

// per-world episode state of an armed manager (reset_worlds_kernel)
struct ResetArgs {
    int32_t *flag;      // [W] MBOTS_EXPORT_RESET: 0 none, 1 next episode, v >= 2 episode v - 2
    int32_t *episode;   // [W] the world's current episode
    int32_t *age;       // [W] steps since the world's last reset or creation
    uint32_t len;       // episode length in steps (0: off)
    int32_t *mark;      // [W] 1: this pass re-initialised the world, else 0 (the trajectory
                        // window's push copies it)
};

// the small kernel class of mixed-class dispatch
constexpr int kSmallCap = 128;
// a world whose next K1 needs the class kernel: it may end with 2 n + A agents
__host__ __device__ inline bool k1_needs_class(int n, uint32_t A) { return 2 * n + (int)A > kSmallCap; }

inline void swap_state(SimState &S)
{
    auto sw = [](auto &a, auto &b) { auto t = a; a = b; b = t; };
    sw(S.x, S.x_out); sw(S.y, S.y_out); sw(S.rw, S.rw_out); sw(S.rz, S.rz_out);
    sw(S.species, S.species_out); sw(S.n, S.n_out);
    sw(S.food, S.food_out);
}

// One half of the double-buffered species-major observation table
// (AgentObservationArchetype, types.hpp:228-252, + raycast output columns).
struct ObsTable {
    int32_t *species;  float *pos;  int32_t *health;  float *sur;  float *reward;
    int32_t *action;   int32_t *stats;  float *hidden;  int8_t *sem;  uint8_t *depth;
    int32_t *pspecies; float *ppos; int32_t *phealth; float *psur; float *preward;
    int32_t *paction;  int32_t *pstats; float *phidden; int8_t *psem; uint8_t *pdepth;
};

constexpr int kTotRows = 5;   // totals[kTotRows]: rows the moves / shift / checkpoints cover
constexpr int kTotMaxPop = 8;     // totals_host[kTotMaxPop + tile]: the tile's largest world
                                  // population after the last K2 (the pinned mirror only)
constexpr int kTotOverflow = 6;   // totals[kTotOverflow]: births / respawns dropped at the
                                  // capacity cap so far (exported worlds; K1 adds, K2 mirrors)
uint32_t scan_tiles(uint32_t W);
// whether the sensor renders worlds in K2's population order (every scan tile
// full)
bool sensor_order_used(uint32_t W);
// K1 blocks add their counts into one of kTileBuckets copies of their tile's
// counters (block index mod 8): fewer same-address atomics at K1's end
constexpr int kTileBuckets = 8;
hipError_t launch_init(const SimState &S, hipStream_t st);
// the reset pass of an armed manager, before K1 on K1's stream: flagged or
// expired worlds re-initialised in the state half K1 reads (parity: this
// step's; mixed classes: the K1 class list K1 reads is rebuilt from the new
// populations)
hipError_t launch_reset_worlds(const SimState &S, const ResetArgs &R, int parity, hipStream_t st);
// flag[w] = v[w] wherever v[w] != 0 (mbots_reset_worlds)
hipError_t launch_set_flags(int32_t *flag, const int32_t *v, uint32_t W, hipStream_t st);
// the sensor's ray table (host-computed with the kernels' own u_of / near_pt)
hipError_t upload_ray_table(const SimState &S, hipStream_t st);
hipError_t launch_tile_sum(const SimState &S, int parity, hipStream_t st);
hipError_t launch_raise_flag(uint32_t *flag, uint32_t v, hipStream_t st);
hipError_t launch_world_step(const SimState &S, const ObsTable &cur, int parity, hipStream_t st,
                             hipEvent_t done = nullptr);
// plain_events: record `done` with hipEventRecord (stream capture) instead of on the dispatch
hipError_t launch_scan(const SimState &S, int parity, hipStream_t st, hipEvent_t done = nullptr,
                       bool plain_events = false);
// mixed classes: the K1 class list of slot `slot` rebuilt from S.n (after a
// checkpoint load; K2 builds it every step)
hipError_t launch_build_lists(const SimState &S, int slot, hipStream_t st);
hipError_t launch_export_rows(const SimState &S, const ObsTable &nxt, int init, hipStream_t st);
// K4 parts (DESIGN.md "Deferred Prev moves"): Action + HiddenState; the same
// also into PrevAction / PrevHiddenState (the fused shift); the prev sensor;
// PrevAction / PrevHiddenState; the six other Prev* columns
constexpr int kMoveAH = 1, kMoveAHShift = 2, kMoveSensor = 4, kMovePrevAH = 8, kMovePrev6 = 16;
constexpr int kMoveAll = kMoveAH | kMoveSensor | kMovePrevAH | kMovePrev6;
// (lazy_rows, with kMoveAHShift: the lazy shift -- Action only, and the row
// count stored there for launch_materialize_hidden)
hipError_t launch_move(const SimState &S, const ObsTable &cur, const ObsTable &nxt, int prev_lazy,
                       int parts, hipStream_t st, uint32_t *lazy_rows = nullptr);
// dst[r] = base[map[r]] (0 where map[r] < 0) for r < *rows: 64 B rows
hipError_t launch_materialize_hidden(const SimState &S, const uint32_t *rows, const int32_t *map, const float *base,
                                     float *dst, hipStream_t st);
// the same over 24 B Action rows (owed PrevAction: map is a step's src_of)
hipError_t launch_materialize_action(const SimState &S, const uint32_t *rows, const int32_t *map, const int32_t *base,
                                     int32_t *dst, hipStream_t st);
hipError_t launch_sensor(const SimState &S, const ObsTable &nxt, hipStream_t st,
                         hipEvent_t done = nullptr, bool plain_events = false);
// shift modes: every Prev* column / Action + HiddenState only (lazy) / the six
// columns a lazy shift left (materialise)
constexpr int kShiftAll = 0, kShiftEager = 1, kShiftRest = 2;
hipError_t launch_shift(const SimState &S, const ObsTable &t, int mode, hipStream_t st);
hipError_t launch_synthetic_actions(const SimState &S, const ObsTable &t, uint32_t seed,
                                    uint32_t step, int write_hidden, hipStream_t st);
hipError_t launch_sensor_index(const SimState &S, int32_t *out, hipStream_t st);
// six_src: the other half, when the current half's six Prev* columns are
// still the step's deferred move (prev rows gather their three columns along
// src_of, as the move would; six_lazy: that move's source is its current ones)
hipError_t launch_construct_obs(const SimState &S, const ObsTable &t, int prev, int prev_lazy,
                                float *out, uint32_t out_rows, hipStream_t st,
                                const ObsTable *six_src = nullptr, int six_lazy = 0);
// rollout records of the config-5 gather (MBOTS_ROLLOUT_BYTES[_DEPTH])
constexpr uint32_t kRolloutBytes = 64, kRolloutBytesDepth = 96;
hipError_t launch_pack_rollout(const SimState &S, const ObsTable &t, void *out, uint32_t out_rows,
                               hipStream_t st);
hipError_t launch_unpack_rollout(const void *recs, uint32_t n, int fixd, float *obs, float *reward,
                                 int32_t *stats, hipStream_t st);
// learner records of the config-5 round trip (MBOTS_LEARNER_BYTES[_DEPTH])
constexpr uint32_t kLearnerBytes = 272, kLearnerBytesDepth = 336;
// `t` holds every logical column's storage (the manager materialised the
// step's deferred moves); prev_lazy: the six Prev* columns are the current ones
hipError_t launch_pack_learner(const SimState &S, const ObsTable &t, int prev_lazy, void *out, uint32_t out_rows,
                               hipStream_t st);
hipError_t launch_unpack_learner(const void *recs, uint32_t n, int fixd, const mbots_learner_out &o,
                                 hipStream_t st);
// slim learner records (MBOTS_LEARNER_SLIM_BYTES[_DEPTH]): `t` the current half
// (prev_lazy: its six Prev* columns are the current ones); the previous
// observation columns the step still owes are gathered along S.src_of inside
// the launch -- the six from `six_src` (six_lazy: from its current columns),
// the prev sensor from `sem_src`'s sensor rows -- when those are non-null
constexpr uint32_t kLearnerSlimBytes = 128, kLearnerSlimBytesDepth = 192;
hipError_t launch_pack_learner_slim(const SimState &S, const ObsTable &t, int prev_lazy, const ObsTable *six_src,
                                    int six_lazy, const ObsTable *sem_src, void *out, uint32_t out_rows,
                                    hipStream_t st);
hipError_t launch_unpack_learner_slim(const void *recs, uint32_t n, int fixd, const mbots_learner_out &o,
                                      int32_t *src, hipStream_t st);
// the learner rank's rebuild of Action / HiddenState / PrevHiddenState from
// slim records' provenance (mbots_rebuild_learner): per (rank, species) the
// first global row of the gathered table, and of the last table with the
// owning rank's local first row
struct RebuildPlan {
    int32_t ranks;
    int32_t sp_end[4];                                  // gathered table: species segment ends
    int32_t cur_g[MBOTS_MAX_LEARNER_RANKS][4];          // gathered: first global row of (rank, species)
    int32_t last_l[MBOTS_MAX_LEARNER_RANKS][4];         // last table: first local row of (rank, species)
    int32_t last_g[MBOTS_MAX_LEARNER_RANKS][4];         // last table: its first global row
};
RebuildPlan rebuild_plan(const int64_t *cur_counts, const int64_t *last_counts, uint32_t ranks);
// global row of the last table for gathered row r with provenance o (-1: none)
__host__ __device__ inline int32_t rebuild_row(const RebuildPlan &p, int32_t r, int32_t o)
{
    if (o < 0) return -1;
    int s = 0;
    while (s < 3 && r >= p.sp_end[s]) ++s;
    int k = 0;
    while (k + 1 < p.ranks && r >= p.cur_g[k + 1][s]) ++k;
    int t = 3;
    while (t > 0 && o < p.last_l[k][t]) --t;
    return p.last_g[k][t] + (o - p.last_l[k][t]);
}
// capacity growth (mbots_grow_capacity): the per-slot columns ([world][cap],
// 4-byte slots) re-laid from cap_old to cap_new slots per world in one launch,
// the new slots [cap_old, cap_new) of every world zeroed
constexpr int kGrowCols = 11;
struct GrowCols {
    const void *src[kGrowCols];
    void *dst[kGrowCols];
};
hipError_t launch_grow_slots(const GrowCols &c, uint32_t W, uint32_t cap_old, uint32_t cap_new, hipStream_t st);
hipError_t launch_rebuild_learner(const RebuildPlan &p, const int32_t *src, uint32_t rows, uint32_t last_rows,
                                  const int32_t *last_action, const float *last_memory, const float *last_hidden,
                                  int32_t *action, float *hidden, float *prev_hidden, hipStream_t st);

// trajectory window (mbots_traj.hpp): the push of the current table (`reward`:
// its Reward column; `value`: N f32 or null; reset_mark: the last reset pass's
// marks or null) into ring slot `slot`, and compute's three launches over the
// n pushed tables (max_count: the largest N_t, at most max_rows)
hipError_t launch_traj_push(const SimState &S, const TrajWin &w, uint32_t slot, const float *reward,
                            const float *value, const int32_t *reset_mark, hipStream_t st);
hipError_t launch_traj_compute(const TrajWin &w, const TrajParams &P, uint32_t n, uint32_t max_count, hipStream_t st);
// the window's opt-in parts: the push of HiddenState and the Action mask (`t`:
// the current table as its readers see it); the numbering of the sequences of
// the n computed tables (count, scan, walk; the total lands in
// w.blk[horizon * ceil(max_rows / 256)]); a batch of the sequences
// [lo, lo + B) -- padding fills, the scatter and, with `obs`, the record
// decode, which reads o.rows / o.t0 --; and the gather of the caller's own
// per-table rows (`tables`: n device pointers in device memory) along a
// batch's rows / t0
hipError_t launch_traj_push_state(const SimState &S, const TrajWin &w, uint32_t slot, const ObsTable &t,
                                  hipStream_t st);
hipError_t launch_traj_sequences(const TrajWin &w, uint32_t n, uint32_t max_count, hipStream_t st);
hipError_t launch_traj_batch(const TrajWin &w, const TrajBatch &o, uint32_t lo, uint64_t B, uint32_t n,
                             uint32_t max_count, float *obs, hipStream_t st);
hipError_t launch_traj_gather(const int32_t *rows, const int32_t *t0, uint64_t B, uint32_t n,
                              const void *const *tables, uint32_t row_bytes, void *out, hipStream_t st);

// rasteriser (mbots_render.hpp): k images of 96 scale x 128 scale pixels in one
// launch, image i of world worlds[i] (device memory; null: world i) as the
// state stands in stream order; out's non-null arrays receive them
hipError_t launch_render(const SimState &S, const uint32_t *worlds, uint32_t k, uint32_t scale, const RenderOut &out,
                         hipStream_t st);

// device actor (mbots_policy.hpp; kernels in mbots_policy.hip): one persistent
// launch over every table row (the shard ghost's included) of the current
// table `t` -- hidden_in: its HiddenState column as readers see it; flags:
// kActGreedy / kActNoWrite; draw: the device's draw counter; the [out_rows]
// outputs may be null; max_rows: the table's row slots --, the counter's
// advance, the upload of a net's layers into fragment order, and the
// activations of mbots_policy_activation.  groups null: one group, the four
// nets of `nets` by value; else the groups' net table (`nets` unused).  gated:
// a net of the launch has a gate head (the kernels with the gate's code).
// launch_policy_segments: out [G][4][2], the exported rows of every (group,
// species) of the current table
hipError_t launch_policy_act(const SimState &S, const ObsTable &t, const float *hidden_in, const PolNets &nets,
                             const PolGroups *groups, bool gated, uint32_t flags, const uint32_t *draw,
                             int32_t *action_out, float *logp_out, float *value_out, uint32_t out_rows,
                             uint32_t max_rows, hipStream_t st);
hipError_t launch_policy_segments(const SimState &S, const PolGroups &groups, int32_t *out, hipStream_t st);
hipError_t launch_policy_draw_next(uint32_t *draw, hipStream_t st);
hipError_t launch_policy_repack(const PolUploads &U, hipStream_t st);
hipError_t launch_policy_activation(int act, const float *x, float *y, uint64_t n, hipStream_t st);
// evaluate and its backward pass (mbots_policy.hpp): `net` in fragment order,
// `back` its transposed layers (trunk 1.., heads) in fragment order with +0
// biases; the backward's persistent launch has slabs.nacc blocks, each with
// kPolStashTiles tiles of `stash`, and is followed by the reduce into `out`
hipError_t launch_policy_eval(const PolEvalIO &io, const PolNet &net, hipStream_t st);
size_t policy_grad_stash_floats(uint32_t nacc);
hipError_t launch_policy_grad(const PolEvalIO &io, const PolNet &net, const PolNet &back, const PolGradSlabs &slabs,
                              float *stash, const PolGradOut &out, hipStream_t st);
// grouped evaluate (mbots_policy.hpp): the 4 G nets of `specs` (host memory; the
// specs travel as kernel arguments) described into `table` and repacked into
// `ws` by way of `uploads` (nseg * kPolGroupUploads entries), then one forward
// launch over the segments' tiles; or the backward in `nwaves` waves, wave w
// the segments waves[w] with a grid of (wave_acc, waves[w].n) blocks -- block
// (a, c) on slab and stash c * wave_acc + a -- followed by its reduce into
// grads[w].  `segments` [nseg][2] is read on the device only.
hipError_t launch_policy_eval_groups(const PolEvalIO &io, const int32_t *segments, const PolGroupSpec *specs,
                                     uint32_t nseg, float *ws, PolGroupEntry *table, PolUpload *uploads, hipStream_t st);
hipError_t launch_policy_grad_groups(const PolEvalIO &io, const int32_t *segments, const PolGroupSpec *specs,
                                     uint32_t nseg, const PolGroupWave *waves, const PolGroupGrads *grads,
                                     uint32_t nwaves, float *ws, PolGroupEntry *table, PolUpload *uploads, float *slabs,
                                     uint64_t slab_stride, float *stash, uint32_t wave_acc, hipStream_t st);
// evaluate_sequences and its backward pass through time (mbots_policy.hpp): as
// above with the memory head in `net`, its transpose in back.memory, and in
// back.trunk[0] the H -> 16 layer over the first layer's HiddenState columns;
// hws: pol_seq_h_floats(slabs.nacc, io.L) floats, the h_k of a block's tile
hipError_t launch_policy_seq_eval(const PolSeqIO &io, const PolNet &net, hipStream_t st);
hipError_t launch_policy_seq_grad(const PolSeqIO &io, const PolNet &net, const PolNet &back, const PolGradSlabs &slabs,
                                  float *stash, float *hws, const PolGradOut &out, hipStream_t st);
// grouped evaluate_sequences (mbots_policy.hpp): launch_policy_eval_groups'
// arguments for nets with a memory head (nseg * kPolSeqGroupUploads repack
// entries), the columns through `order`; the backward's waves also share `hws`,
// kPolGroupWave * wave_acc h stores of [L][64][16]
hipError_t launch_policy_seq_eval_groups(const PolSeqIO &io, const int32_t *order, const int32_t *segments,
                                         const PolSeqGroupSpec *specs, uint32_t nseg, float *ws, PolGroupEntry *table,
                                         PolUpload *uploads, hipStream_t st);
hipError_t launch_policy_seq_grad_groups(const PolSeqIO &io, const int32_t *order, const int32_t *segments,
                                         const PolSeqGroupSpec *specs, uint32_t nseg, const PolGroupWave *waves,
                                         const PolSeqGroupGrads *grads, uint32_t nwaves, float *ws, PolGroupEntry *table,
                                         PolUpload *uploads, float *slabs, uint64_t slab_stride, float *stash, float *hws,
                                         uint32_t wave_acc, hipStream_t st);
// sequence_segments: the columns sorted by net_id (stable, nkeys <= 256 keys)
// into `order` [B] and their [lo, hi) into `segments` [nkeys][2]; `counts` holds
// policy_seq_order_workspace(B) bytes
size_t policy_seq_order_workspace(uint64_t B);
hipError_t launch_policy_seq_order(const int32_t *net_id, uint64_t B, uint32_t nkeys, int32_t *order, int32_t *segments,
                                   uint32_t *counts, hipStream_t st);
// the update on the device (mbots_policy.hpp): the groups' row totals; the
// loss, one block per group after a fill of the three gradients with +0; Adam
// over `tensors` (host memory) in launches of kAdamTensors descriptors each,
// then the one-block launch that advances the active groups' state
hipError_t launch_policy_group_rows(const int32_t *segments, uint32_t groups, int64_t *rows, hipStream_t st);
hipError_t launch_policy_a2c_loss(const PolLossIO &io, uint32_t groups, hipStream_t st);
hipError_t launch_policy_adam(const AdamTensor *tensors, uint64_t count, AdamState *state, uint32_t groups,
                              const int64_t *rows, const AdamCoef &C, hipStream_t st);
// the same for the padded [L, B] sequence batches: every group's kept elements
// (io's len, t0, end, order, segments, B and last_table); the loss, one block
// per group after the fill
hipError_t launch_policy_seq_group_rows(const PolSeqLossIO &io, uint32_t groups, int64_t *rows, hipStream_t st);
hipError_t launch_policy_seq_a2c_loss(const PolSeqLossIO &io, uint32_t groups, hipStream_t st);
// Adam with the groups' gradient norms, clipping and weight decay: per launch
// of kAdamTensors descriptors the chunks' squared norms and their fold; the
// groups' norms and clip factors; the element launches; the state's advance.
// `workspace`: pol_adam_clip_bytes of policy_adam_clip_counts' two numbers
void policy_adam_clip_counts(const AdamTensor *tensors, uint64_t count, uint64_t &chunks, uint64_t &present);
hipError_t launch_policy_adam_clip(const AdamTensor *tensors, uint64_t count, AdamState *state, uint32_t groups,
                                   const int64_t *rows, const AdamCoef &C, const AdamClipCoef &K, float *grad_norm,
                                   void *workspace, hipStream_t st);
// PPO on the device (mbots_policy.hpp): one block per (group, species, chunk)
// leaves the chunk's partials in io.part, a one-block-per-group launch folds
// them into io.out in the fixed order; the loss follows a fill of the three
// gradients with +0.  The gate: one block, thread per group
hipError_t launch_policy_adv_moments(const PolPpoIO &io, uint32_t groups, hipStream_t st);
hipError_t launch_policy_ppo_loss(const PolPpoIO &io, uint32_t groups, hipStream_t st);
hipError_t launch_policy_seq_adv_moments(const PolSeqPpoIO &io, uint32_t groups, hipStream_t st);
hipError_t launch_policy_seq_ppo_loss(const PolSeqPpoIO &io, uint32_t groups, hipStream_t st);
hipError_t launch_policy_ppo_gate(const double *stats, const int64_t *rows, double target_kl, int64_t *gate,
                                  uint32_t groups, hipStream_t st);

}  // namespace mbots
