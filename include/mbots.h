/*
 * mbots.h -- C ABI of the MI355X-native madrona-bots simulator (libmbots.so).
 *
 * This is the drop-in boundary for the reference's host surface:
 *   class Manager            src/entry/mgr.hpp:10-68
 *   Manager::Impl::make      src/entry/mgr.cpp:98-172
 *   nanobind SimManager      src/entry/entry.cpp:16-45
 * Plain pointers, sizes and status codes only (no torch / HIP C++ types).
 * Every function returns MBOTS_OK (0) or a negative MBOTS_E* code; the text of
 * the last error on the calling thread is available from mbots_last_error().
 * The one positive status is mbots_step's MBOTS_W_CAPACITY (a warning: the
 * step ran).
 * Streams are passed as `void *` holding a hipStream_t (NULL = default stream;
 * ignored in MBOTS_EXEC_CPU mode, where every call completes before returning).
 *
 * Ownership (mgr.cpp:70-76): the handle owns every device buffer; tensors
 * returned by mbots_export are non-owning views that stay valid until the next
 * mbots_step (the export tables are double-buffered and swap on every step;
 * the reference's views are likewise shape-stale after step()).
 */
#ifndef MBOTS_H
#define MBOTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBOTS_OK             0
#define MBOTS_E_INVALID    (-1)   /* bad argument / config             */
#define MBOTS_E_HIP        (-2)   /* HIP runtime error                  */
#define MBOTS_E_NOMEM      (-3)   /* device / host allocation failed    */
#define MBOTS_E_RANGE      (-4)   /* index out of range                 */
#define MBOTS_E_CAPACITY   (-5)   /* mbots_step with MBOTS_FLAG_STRICT_CAPACITY:
                                     agents were dropped at agent_capacity (the
                                     step ran; see MBOTS_W_CAPACITY) */
/* mbots_step warning (the step ran): since the last report, births or
 * respawns were dropped because a world had reached agent_capacity.  The
 * reference's tables have no cap (makeAgent in healthSync and in the respawn,
 * sim.cpp:561-564, :830-834), so from that step on the run diverges from the
 * reference's.  Reported from the row counts the device last published, so
 * it can come a few steps after the drop (once per rise of mbots_overflow). */
#define MBOTS_W_CAPACITY     1

/* Manager::Config flags (build extensions; default 0 = reference-faithful) */
#define MBOTS_FLAG_REWARD_FIXED     0x1u  /* rewards[speciesID-1] (fixes sim.cpp:943) */
#define MBOTS_FLAG_FIX_DEPTH_ALIAS  0x2u  /* depth_tensor exports real depth (sim.cpp:102-112) */
/* shard ghost: also step world world_offset + num_worlds (the next shard's
 * first world), never exported, so the faithful rewards[speciesID] of the
 * shard's last world reads the same SpeciesInfo row as on one device
 * (sim.cpp:943).  The ghost's agents act on what
 * mbots_write_synthetic_actions writes (the identity-keyed stream is keyed by
 * global world, so with it N shards == one device exactly); its rows lie past
 * row N, outside every exported view, so a learner writing actions through
 * the views leaves them to replay their last actions (carried through the row
 * moves and the shift like every row's).  Every shard but the last sets it. */
#define MBOTS_FLAG_SHARD_GHOST      0x4u
/* a capacity drop (MBOTS_W_CAPACITY) is an error: mbots_step returns
 * MBOTS_E_CAPACITY instead */
#define MBOTS_FLAG_STRICT_CAPACITY  0x8u

/* agent_capacity: 4..4096 slots per world (MBOTS_MAX_CAPACITY); the kernel
 * classes are 128 (default), 256, 512, 1024, 2048 and 4096 slots.  Up to 256 the
 * sensor's per-pixel depth key carries the object order (64 + slot for
 * agents) in the low 9 bits of a 32-bit word; the larger classes keep the same
 * quantised depth and the order in a 64-bit key, so a world renders the same
 * bytes in every class.  The K1 finder mode (<= 2048 worlds) is a <= 256-slot
 * mode. */
#define MBOTS_MAX_CAPACITY          4096u

/* execution modes (madrona::ExecMode; the reference's callers pick CPU when
 * no GPU is present, learn/env.py:12-15) */
#define MBOTS_EXEC_HIP  0   /* gfx950 kernels on device gpu_id (default)     */
#define MBOTS_EXEC_CPU  1   /* host threads; bit-identical results, host views */

/* Manager::Config (src/entry/mgr.hpp:12-23) plus sharding / capacity knobs. */
typedef struct mbots_config {
    int32_t  gpu_id;                    /* gpuID                              */
    uint32_t num_worlds;                /* numWorlds held by this instance    */
    uint32_t rand_seed;                 /* randSeed                           */
    uint32_t init_num_agents_per_world; /* initNumAgentsPerWorld              */
    uint32_t sensor_size;               /* sensorSize; must be 32             */
    uint32_t world_offset;              /* global index of world 0 (shards)   */
    uint32_t agent_capacity;            /* per-world slot cap (0 -> 128)      */
    uint32_t flags;                     /* MBOTS_FLAG_*                       */
    int32_t  exec_mode;                 /* MBOTS_EXEC_* (ExecMode)            */
} mbots_config;

/* Export slots; numbering mirrors enum class ExportID (src/sim/sim.hpp:18-55). */
enum mbots_export_id {
    MBOTS_EXPORT_RESET = 0,
    MBOTS_EXPORT_ACTION = 1,
    MBOTS_EXPORT_PREV_ACTION = 2,
    MBOTS_EXPORT_HIDDEN_STATE = 3,
    MBOTS_EXPORT_PREV_HIDDEN_STATE = 4,
    MBOTS_EXPORT_REWARD = 5,
    MBOTS_EXPORT_PREV_REWARD = 6,
    MBOTS_EXPORT_DONE = 7,
    MBOTS_EXPORT_POSITION = 8,
    MBOTS_EXPORT_PREV_POSITION = 9,
    MBOTS_EXPORT_HEALTH = 10,
    MBOTS_EXPORT_PREV_HEALTH = 11,
    MBOTS_EXPORT_SURROUNDING = 12,
    MBOTS_EXPORT_PREV_SURROUNDING = 13,
    MBOTS_EXPORT_SENSOR_SEMANTIC = 14,
    MBOTS_EXPORT_SENSOR_DEPTH = 15,
    MBOTS_EXPORT_PREV_SENSOR_SEMANTIC = 16,
    MBOTS_EXPORT_PREV_SENSOR_DEPTH = 17,
    MBOTS_EXPORT_STATS = 18,
    MBOTS_EXPORT_PREV_STATS = 19,
    MBOTS_EXPORT_SENSOR_INDEX = 20,
    MBOTS_EXPORT_SPECIES_COUNT = 21,
    MBOTS_EXPORT_NUM_REFERENCE = 22,
    /* build extensions (not exported by the reference) */
    MBOTS_EXPORT_SPECIES = 32,           /* SpeciesObservation column     */
    MBOTS_EXPORT_PREV_SPECIES = 33,      /* PrevSpeciesObservation column */
    MBOTS_EXPORT_EPISODE = 34,           /* int32 [num_worlds, 1]: the world's episode   */
    MBOTS_EXPORT_EPISODE_STEP = 35       /* int32 [num_worlds, 1]: steps since its last
                                            reset or creation                            */
};

/* element types (madrona::py::TensorElementType subset) */
enum mbots_dtype {
    MBOTS_DTYPE_UINT8 = 0,
    MBOTS_DTYPE_INT8 = 1,
    MBOTS_DTYPE_INT32 = 2,
    MBOTS_DTYPE_FLOAT32 = 3
};

/* A non-owning 2-D tensor view (madrona::py::Tensor, mgr.cpp:70-76). */
typedef struct mbots_tensor {
    void   *data;        /* device pointer                                  */
    int32_t dtype;       /* enum mbots_dtype                                */
    int32_t device;      /* HIP device ordinal (gpuID); -1: host memory (CPU mode) */
    int64_t dims[2];     /* rows, columns                                   */
} mbots_tensor;

typedef struct mbots_handle mbots_handle;

/* Manager::Manager / Impl::make (mgr.cpp:98-172, :180-183).  Runs world init
 * (Sim::Sim, sim.cpp:1232-1256) and the Init graph (sim.cpp:1050-1059). */
int mbots_create(const mbots_config *cfg, mbots_handle **out);
/* Manager::~Manager (mgr.cpp:185-187) */
int mbots_destroy(mbots_handle *h);

/* Manager::step (mgr.cpp:51-63, :189-192): Step + Sensor graphs, enqueued on
 * `stream`.  Unlike the reference it does not block; mbots_num_agents and the
 * host-side offsets synchronise with the last step on demand. */
int mbots_step(mbots_handle *h, void *stream);
/* Manager::shiftObservations (mgr.cpp:65-68, :194-197) */
int mbots_shift_observations(mbots_handle *h, void *stream);

/* SimBridge::totalNumAgents (sim.hpp:74-78, sim.cpp:992-993).  Waits for the
 * last step's counters. */
int mbots_num_agents(mbots_handle *h, uint32_t *out);
/* Manager::exportTensor / the 11 tensor accessors (mgr.cpp:70-76, :199-422).
 * The reference's step() is synchronous (mgr.cpp:51-63), so its views are
 * valid on any stream; mbots_export keeps that contract: it returns after the
 * view's data is final (host-synchronising with the manager's last stream). */
int mbots_export(mbots_handle *h, int32_t export_id, mbots_tensor *out);
/* Stream-ordered form (what the Python surface uses): any deferred copy or
 * join the view needs is enqueued on `stream`, after everything the manager
 * enqueued on the stream of its previous call, so the view's data is final in
 * stream order on `stream`.  The view's row count (dims[0] = N) is host
 * state: the first call after a step waits once on the host for that step's
 * row counts (mbots_num_agents); the data copies and joins themselves do not
 * synchronise the host.  MBOTS_EXPORT_SENSOR_INDEX is computed on `stream`
 * and synchronised before returning. */
int mbots_export_on(mbots_handle *h, int32_t export_id, void *stream, mbots_tensor *out);
/* Manager::setAction (mgr.cpp:251-272): row = export row (species-major). */
int mbots_set_action(mbots_handle *h, uint32_t row, const int32_t action[6]);
/* Manager::agentOffsetForWorld (mgr.cpp:274-277) */
int mbots_agent_offset_for_world(mbots_handle *h, uint32_t world, uint32_t *out);

/* Learner observation rows (learn/util.py:14-29 construct_obs over every
 * species at once): out (device, >= out_rows x 69 f32, row-major) receives rows
 * [0, min(N, out_rows)) of [depth 32 | health 1 | position 2 | semantic 32 |
 * surrounding 2], exactly torch.cat's promotion of the exported views
 * (prev != 0: the Prev* views).  Launched on `stream` after the sensor rows. */
int mbots_construct_obs(mbots_handle *h, int32_t prev, float *out, uint64_t out_rows,
                        void *stream);

/* Rollout records for the learner-rank gather (BASELINE config 5):
 * the raw columns the reference's training loop reads after step()
 * (learn/training_loop.py:43-57, :87; learn/util.py:14-29), one fixed-size
 * record per export row, so a rank ships ~64 B per agent instead of the 276-B
 * f32 learner row:
 *   bytes  0..31  semantic (int8 x 32)        32..35  health (int32 bits)
 *         36..43  position (f32 x 2)          44..51  surrounding (f32 x 2)
 *         52..55  reward (f32)                56..59  stats (4 x uint8 flags)
 *         60..63  zero
 *         64..95  depth (uint8 x 32), only with MBOTS_FLAG_FIX_DEPTH_ALIAS
 * mbots_pack_rollout writes rows [0, min(N, out_rows)) into `out` (device
 * memory of the manager's GPU, 16-byte aligned; host memory in CPU mode). */
#define MBOTS_ROLLOUT_BYTES        64u
#define MBOTS_ROLLOUT_BYTES_DEPTH  96u
int mbots_rollout_record_bytes(mbots_handle *h, uint32_t *out);
int mbots_pack_rollout(mbots_handle *h, void *out, uint64_t out_rows, void *stream);
/* Learner side, no manager needed: `rows` gathered records (with_depth: the
 * 96-B form) -> obs [rows, 69] f32 exactly as mbots_construct_obs builds them,
 * reward [rows] f32 and stats [rows, 4] int32 (either may be NULL; records
 * and stats 16-B aligned on the device).  device >= 0: pointers are device memory of that GPU and the
 * kernel runs on `stream`; device == -1: host memory, done before returning. */
int mbots_unpack_rollout(const void *records, uint64_t rows, int32_t with_depth, int32_t device,
                         float *obs, float *reward, int32_t *stats, void *stream);

/* Learner records: the config-5 round trip (BASELINE config 5, SURVEY 8e
 * steps 1-3).  Everything learn/training_loop.py reads between step() and its
 * writes -- the rollout record above (current observation columns, reward,
 * stats: :49-50, :58), the previous observation columns (:87), Action (:47,
 * :93), HiddenState (:48, :58) and PrevHiddenState (:89) -- one record per
 * export row:
 *   bytes   0..63   the rollout record (bytes 60..63 zero)
 *          64..95   prev semantic        96..99   prev health (int32 bits)
 *         100..107  prev position       108..115  prev surrounding
 *         116..139  Action (int32 x 6)  140..143  zero
 *         144..207  HiddenState (f32 x 16)
 *         208..271  PrevHiddenState (f32 x 16)
 *         272..335  depth, prev depth (uint8 x 32 each), only with
 *                   MBOTS_FLAG_FIX_DEPTH_ALIAS
 * mbots_pack_learner writes rows [0, min(N, out_rows)) into `out` (16-byte
 * aligned device memory; host memory in CPU mode). */
#define MBOTS_LEARNER_BYTES        272u
#define MBOTS_LEARNER_BYTES_DEPTH  336u
int mbots_learner_record_bytes(mbots_handle *h, uint32_t *out);
int mbots_pack_learner(mbots_handle *h, void *out, uint64_t out_rows, void *stream);
/* Learner side (no manager): records -> any of these (NULL: skipped); obs and
 * prev_obs are construct_obs rows of the current / previous columns
 * (learn/util.py:14-29, bit-identical). */
typedef struct mbots_learner_out {
    float   *obs;          /* [rows, 69] */
    float   *prev_obs;     /* [rows, 69] */
    float   *reward;       /* [rows]     */
    int32_t *stats;        /* [rows, 4]  */
    int32_t *action;       /* [rows, 6]  */
    float   *hidden;       /* [rows, 16] */
    float   *prev_hidden;  /* [rows, 16] */
} mbots_learner_out;
int mbots_unpack_learner(const void *records, uint64_t rows, int32_t with_depth, int32_t device,
                         const mbots_learner_out *out, void *stream);
/* Slim learner records (config 5 with row provenance): the
 * learner record without Action, HiddenState and PrevHiddenState -- 152 B of
 * the 272 that only echo what the learner rank itself wrote (training_loop.py
 * :136-137) one and two steps back, reordered by the species sort.  In their
 * place the record carries each row's provenance: src, the row's index in the
 * table before this step (-1: born or respawned this step), from which the
 * learner rank rebuilds the three columns (harness/gather.py LearnerState):
 *   bytes   0..59   as the learner record       60..63   src (int32)
 *          64..115  as the learner record (the previous observation columns)
 *         116..127  zero
 *         128..191  depth, prev depth (uint8 x 32 each), only with
 *                   MBOTS_FLAG_FIX_DEPTH_ALIAS
 * The rebuilt columns equal the manager's as long as every row's Action and
 * HiddenState were written after the last step, after its shift(s) (the
 * learner's loop: step, gather, shift, write).  mbots_pack_learner_slim
 * moves none of the step's deferred columns: the previous observation rows
 * the step still owes are gathered inside its launch. */
#define MBOTS_LEARNER_SLIM_BYTES        128u
#define MBOTS_LEARNER_SLIM_BYTES_DEPTH  192u
int mbots_pack_learner_slim(mbots_handle *h, void *out, uint64_t out_rows, void *stream);
/* records -> obs, prev_obs, reward, stats of `out` (its action / hidden /
 * prev_hidden must be NULL) and src [rows] int32 (may be NULL) */
int mbots_unpack_learner_slim(const void *records, uint64_t rows, int32_t with_depth, int32_t device,
                              const mbots_learner_out *out, int32_t *src, void *stream);
/* The learner rank's rebuild from slim records (no manager): for every row r
 * of the gathered global table (species-major, per species rank-major: the
 * reassembly of harness/gather.py) with provenance src[r] (the owning rank's
 * row before the step, -1 new), its row g in the last global table, then
 *   action[r] = last_action[g], hidden[r] = last_memory[g],
 *   prev_hidden[r] = last_hidden[g]            (zeros for src = -1)
 * -- the learner's own writes after the last step and that step's
 * HiddenState, moved as the species sort moved the rows.  cur_counts /
 * last_counts: [ranks][4] species rows per rank of the gathered / the last
 * table (host memory, ranks <= MBOTS_MAX_LEARNER_RANKS).  device >= 0:
 * every array is device memory of that GPU (16-B aligned), on `stream`;
 * device == -1: host memory. */
#define MBOTS_MAX_LEARNER_RANKS 32u
int mbots_rebuild_learner(const int32_t *src, uint64_t rows, const int64_t *cur_counts,
                          const int64_t *last_counts, uint32_t ranks, const int32_t *last_action,
                          const float *last_memory, const float *last_hidden, uint64_t last_rows,
                          int32_t *action, float *hidden, float *prev_hidden, int32_t device,
                          void *stream);
/* The learner's writes (training_loop.py:136-137: action_tensor[...] = one_hot,
 * memory_tensor[...] = new_memory) for every row at once: `rows` rows of
 * Action [rows, 6] int32 and/or HiddenState [rows, 16] f32 (either may be
 * NULL) from memory of the manager's device (host memory in CPU mode) into
 * the current export table, rows [0, rows).  rows is N, or mbots_num_rows()
 * to also write the shard ghost's rows (the next shard's first world, which
 * then acts exactly as on the next rank). */
int mbots_write_actions(mbots_handle *h, const int32_t *action, const float *hidden, uint64_t rows,
                        void *stream);
/* every table row: N plus the shard ghost's (which follow row N) */
int mbots_num_rows(mbots_handle *h, uint32_t *out);
/* the largest world population after the last step (the shard ghost
 * included): waits for that step's row counts only (K2), not for its sensor
 * or the caller's chain -- what mbots_set_auto_capacity checks before each
 * step (a step adds at most n births and A respawns) */
int mbots_max_population(mbots_handle *h, uint32_t *out);

/* Checkpoint / restore (the reference has none): the live state
 * after the last step (agent SoA, RNG keys/counters, food, the current export
 * table's N rows) as a host blob.  A manager created with the same
 * configuration continues bit-exactly after mbots_load_checkpoint -- also
 * one of another agent_capacity, when every world of the blob fits it (the
 * per-slot columns are re-laid out; a world that does not fit is refused
 * before anything is overwritten).  The Python SimManager's CPU mode grows a
 * run through the capacity classes this way; HIP mode and C callers grow in
 * place (mbots_grow_capacity below). */
int mbots_checkpoint_size(mbots_handle *h, uint64_t *bytes);
int mbots_save_checkpoint(mbots_handle *h, void *host_dst, uint64_t bytes);
int mbots_load_checkpoint(mbots_handle *h, const void *host_src, uint64_t bytes);

/* Capacity growth in place (the reference's worlds have no population cap,
 * sim.cpp:561-564, :830-834; a manager's have agent_capacity).
 *
 * mbots_capacity: the current slots per world (host state, no
 * synchronisation).
 *
 * mbots_grow_capacity moves the manager into new_capacity slots per world
 * inside the same handle.  Afterwards the manager is indistinguishable from a
 * fresh manager of new_capacity that loaded this manager's checkpoint -- bitwise,
 * on every export and every later step, shift, pack and checkpoint -- except
 * that each row's provenance is carried too, so mbots_pack_learner_slim between
 * the growth and the next step gives the records it gave before the growth.
 * Kernel-timing totals, the agent-step and dropped-agent counters and the
 * MBOTS_W_CAPACITY reporting carry on.  In HIP mode the state moves device to
 * device (one kernel re-lays the per-slot columns, the per-world arrays and
 * the table's live rows are copied; nothing goes through the host), after the
 * device has drained.  new_capacity equal to the current one: MBOTS_OK,
 * nothing done; smaller, or above MBOTS_MAX_CAPACITY, or with
 * (num_worlds + ghost) * new_capacity >= 2^31: MBOTS_E_INVALID (shrinking
 * stays with checkpoints).  MBOTS_E_INVALID also while the manager's stream
 * is being captured, and once any step of this manager has been captured into
 * a graph: captured graphs pin the capacity (a replay writes through the
 * pointers it recorded).  MBOTS_E_NOMEM when the new storage cannot be
 * allocated: the manager is untouched and keeps running at its capacity.
 *
 * Retired storage: a growth does not free the storage it leaves, so a view
 * (mbots_export) taken before it still reads what it read -- but no longer
 * follows the manager; take views again after a growth (their pointers and
 * the column allocations behind them change).  The handle keeps the retired
 * storage until mbots_destroy or mbots_release_retired, after which such
 * views dangle.  Capacity classes double, so everything retired together is
 * smaller than the live storage.
 *
 * mbots_set_auto_capacity(h, 1): mbots_step first reads the largest world
 * population n as mbots_max_population does (a wait for the last step's K2
 * only) and, when 2 n + init_num_agents_per_world exceeds the capacity --
 * the step could overflow -- grows to the smallest class (128, 256, ... 4096)
 * that holds it; at 4096 it stops growing and MBOTS_W_CAPACITY reporting
 * takes over.  A failed growth is returned by mbots_step, which then has not
 * stepped.  mbots_step under stream capture returns MBOTS_E_INVALID while
 * this is enabled: automatic capacity cannot be captured into a graph.  A
 * runtime switch, not a configuration flag: checkpoints of automatic and
 * fixed managers are interchangeable. */
int mbots_capacity(mbots_handle *h, uint32_t *out);
int mbots_grow_capacity(mbots_handle *h, uint32_t new_capacity);
int mbots_set_auto_capacity(mbots_handle *h, int32_t enable);
int mbots_release_retired(mbots_handle *h);
/* Debug dump of one world (viewer replacement): host arrays of agent_capacity
 * rows -- (x, y, rot.w, rot.z) f32, (species, health, finder) i32 -- the 48
 * packed food records, the food boxes' rotations ([5][48] 22-bit quarter-turn
 * fractions; may be NULL) and the live agent count. */
int mbots_world_state(mbots_handle *h, uint32_t world, float *xy_rwrz, int32_t *sp_hp_finder,
                      uint64_t *food, uint32_t *food_rot, int32_t *n_out);
/* The inverse of mbots_world_state for geometry (a debug / test entry point:
 * it puts a chosen scene in front of the sensor): writes the live agents'
 * (x, y, rot.w, rot.z) -- xy_rwrz holds n_agents rows of 4 f32 -- and replaces
 * the world's food by n_food packages, food[k] = (chunk, x, y, 22-bit
 * rotation) with x, y in arena cells as the Python world_state reports them.
 * Each chunk's packages take its slots 0, 1, ... in the order given, and the
 * world's food count follows them.  Population, species, health, finder
 * slots, RNG and the export table stay as they are: the table shows the
 * scene after the next step, and a shoot or breed of that step still acts on
 * the finder slots of the old geometry (in the K1 finder mode on the new
 * one's), so a comparison takes one step without either first.
 * MBOTS_E_INVALID, with the manager untouched, when n_agents differs from the
 * world's population; a coordinate is not finite or outside [0, 127] x
 * [0, 95] (what actionSystem's clamp leaves, sim.cpp:485-486); (rot.w, rot.z)
 * is not finite or |w^2 + z^2 - 1| > 1e-3; a chunk is out of range or holds
 * more than 5 packages, the world more than 30; a package lies outside its
 * chunk's 16 x 16 cells or its rotation is >= 2^22; or the manager's stream
 * is being captured.  HIP mode goes through the checkpoint path (save, patch
 * the blob, load), so the call costs a checkpoint round trip. */
int mbots_set_world_state(mbots_handle *h, uint32_t world, const float *xy_rwrz, uint32_t n_agents,
                          const int32_t *food, uint32_t n_food);

/* Episodes and resets.  The reference registers WorldReset, exports it as
 * ExportID::Reset (sim.cpp:64-75) and seeds a world with
 * split_i(initRandKey, curWorldEpisode++, worldID) (sim.cpp:1236-1240), but its
 * resetSystem is a stub (sim.cpp:302-305); this finishes it with that key
 * schedule: episode e of global world gw is keyed threefry2x32(seed, 0, e, gw),
 * episode 0 being the world mbots_create builds.
 *
 * Reset, then step: a world flagged for reset is re-initialised at the start
 * of the next mbots_step -- exactly as mbots_create initialises it, from its
 * episode's key -- and is then stepped like every other world.  All its agents
 * are new: their rows have no predecessor (Action, HiddenState, every Prev*
 * column and the prev sensor zero, provenance -1, as for a newborn).  The
 * dropped-agent and agent-step counters stay cumulative, the capacity stays,
 * Done stays zeros (derive it from MBOTS_EXPORT_EPISODE_STEP).
 *
 * MBOTS_EXPORT_RESET is the live, writable flag array, one int32 per world:
 * 0 none; 1 reset to the world's next episode (what a learner writes); v >= 2
 * reset to episode v - 2.  The step that consumes a flag clears it.
 * MBOTS_EXPORT_EPISODE is each world's current episode (from 0),
 * MBOTS_EXPORT_EPISODE_STEP the steps since its last reset or creation (1
 * after the step that reset it; counted from 0 again by a checkpoint load that
 * brings no episodes).  All three arrays hold one entry per
 * simulated world: the views show the num_worlds exported worlds, a shard
 * ghost's entry follows at index num_worlds.
 *
 * mbots_reset_worlds flags `n` worlds by global index (episodes NULL: each
 * world's next episode; else episodes[k], < 2^31 - 2, for global_worlds[k]),
 * stream-ordered on `stream`.  Entries outside this manager's worlds are
 * ignored, so every rank of a sharded run can be handed the same list; a rank
 * whose shard ghost is world world_offset + num_worlds resets its ghost from
 * it.  n == 0 does nothing.  MBOTS_E_INVALID while `stream` is being captured
 * (the list is uploaded from the host): under capture, write the flag array.
 *
 * mbots_set_episode_length(h, steps): a world whose MBOTS_EXPORT_EPISODE_STEP
 * has reached `steps` at the start of a step is reset to its next episode, as
 * if its flag were 1 (0: off, the default).  The shard ghost follows the same
 * rule, so shards stay equal to one device with no communication.  Refused
 * once a step of the manager has been captured into a graph.
 *
 * Arming: a manager is unarmed until the first mbots_reset_worlds with n > 0,
 * the first export of MBOTS_EXPORT_RESET or a non-zero episode length; until
 * then mbots_step enqueues exactly what it always did.  An armed manager's
 * steps run the reset pass (one small kernel) before the world step; they stay
 * capturable, and the flag array is read at replay time.  Checkpoints of an
 * armed manager carry the episodes, the ages, the pending flags and the
 * episode length, and arm the manager that loads them; an unarmed manager's
 * checkpoints are unchanged, and loading one into an armed manager starts every
 * world at episode 0, age 0. */
int mbots_reset_worlds(mbots_handle *h, const uint32_t *global_worlds, uint32_t n,
                       const uint32_t *episodes /* NULL: next */, void *stream);
int mbots_set_episode_length(mbots_handle *h, uint32_t steps);

/* Trajectory window: agent lifelines, returns and GAE(lambda) over up to
 * `horizon` consecutive tables.  Every step re-sorts the export table by
 * species, so row r after one step is not row r after the next; the manager
 * alone knows which row an agent came from.  A window records that, per pushed
 * table t and row r < N_t (exported rows only, never the shard ghost's):
 *   MBOTS_TRAJ_LINK    int32  the row of table t - 1 this agent came from (the
 *                             step's own provenance); -1 for a newborn, a
 *                             respawn, any agent of a world re-initialised by
 *                             that step.  Table 0's is recorded, never followed.
 *   MBOTS_TRAJ_REWARD  f32    the Reward column
 *   MBOTS_TRAJ_VALUE   f32    the caller's critic estimate handed to the push
 *   MBOTS_TRAJ_WORLD   int32  the row's global world index
 * and, per world, whether the step that produced table t re-initialised it (an
 * armed manager's reset pass leaves the mark; an unarmed manager has none).
 * A window opened without flags stores no observations: the learner keeps its
 * own tensors in each step's row order and gathers them with these maps (or
 * has the window record and batch them: "Sequences for a recurrent learner"
 * below).
 *
 * A manager holds at most one window; it is off until mbots_traj_open, and a
 * manager that never opens one enqueues in mbots_step exactly what it always
 * did.  The window's storage is its own allocation of 32 bytes per row slot
 * (horizon x max_rows), outside the manager's arena.
 *
 * mbots_traj_push(h, value, stream) records the current table (after
 * mbots_create: the initial one; else the last step's).  value: N_t f32 of
 * the manager's device (host memory in CPU mode) in the table's row order, or
 * NULL for zeros; the launch reads its first min(N_t, max_rows) entries, so a
 * buffer of max_rows entries is always large enough.  It does not synchronise the host: N_t is read from the
 * device's totals inside the launch.  Stream-ordered like every call; it
 * follows the step's export of the rows, not its sensor.  MBOTS_E_INVALID under
 * stream capture and when the window already holds `horizon` tables.  A table
 * of more than max_rows rows is recorded truncated with its true count: the
 * next mbots_traj_compute returns MBOTS_E_RANGE, and keeps doing so until that
 * table has left the window (mbots_traj_clear).
 *
 * mbots_traj_compute(h, gamma, lambda, death_reward, rows_out, n_out, stream)
 * runs over the n pushed tables and fills, for row q of table t:
 *   MBOTS_TRAJ_NEXT (t < n - 1)  the row of table t + 1 holding the same agent
 *                                (the inverse of LINK[t + 1]), or -1
 *   MBOTS_TRAJ_END  int32        0 has a successor; 1 died (no successor, its
 *                                world not re-initialised by step t + 1); 2 cut
 *                                off by a reset of its world; 3 window end
 *                                (t == n - 1)
 *   MBOTS_TRAJ_ADV, MBOTS_TRAJ_RET f32, with r = NEXT[t][q], gl = gamma * lambda
 *   rounded once, and every product and every sum rounded to f32 on its own:
 *     END 0: delta = (REWARD[t+1][r] + gamma * VALUE[t+1][r]) - VALUE[t][q];
 *            ADV = delta + gl * ADV[t+1][r] if t + 1 <= n - 2, else delta
 *     END 1: ADV = death_reward - VALUE[t][q]
 *     END 2: ADV = 0 (neither a next state nor a reward: mask it by END)
 *     RET = ADV + VALUE[t][q];  table n - 1: ADV = 0, RET = VALUE.
 *   With value NULL and lambda 1, RET is the plain discounted return along the
 *   lifeline.  rows_out[0 .. n) (space for `horizon`) receives N_0 .. N_{n-1},
 *   *n_out the table count: the one host synchronisation of the window (on
 *   `stream`, before the launches; the results are final in stream order).  It
 *   may be repeated with other parameters without pushing again.  Both
 *   execution modes give the same bits.  MBOTS_E_INVALID under stream capture
 *   and on an empty window.
 *
 * mbots_traj_clear(h, keep_last) empties the window; keep_last != 0: its
 * newest table becomes table 0 of the next window, so consecutive windows chain
 * without losing a transition (host bookkeeping only: nothing is copied).
 * mbots_load_checkpoint and mbots_set_world_state empty the window too (the
 * rows' provenance is stale after a load); mbots_grow_capacity and automatic
 * growth leave it intact.
 *
 * mbots_traj_view(h, what, t, out): a [N_t, 1] view of one column of table t,
 * valid until the next mbots_traj_clear or mbots_traj_close (a push into a
 * cleared window overwrites it).  The pushed columns can be viewed once the
 * table's row count has reached the host (always in CPU mode, after
 * mbots_traj_compute in HIP mode), the computed ones after a compute of the
 * tables now in the window; else MBOTS_E_INVALID; t outside the window:
 * MBOTS_E_RANGE.  mbots_traj_close frees the window (after the device has
 * drained); every entry point but mbots_traj_open then returns
 * MBOTS_E_INVALID.
 *
 * Sequences for a recurrent learner (all opt-in: mbots_traj_open is
 * mbots_traj_open_ex with flags 0, and such a window keeps its 32 bytes per
 * row slot, its launches and its results).  mbots_traj_open_ex flags:
 *   MBOTS_TRAJ_SEQ        two more int32 columns per row slot (+8 B),
 *                         MBOTS_TRAJ_SEQ_ID and MBOTS_TRAJ_SEQ_POS (views 8, 9),
 *                         and the calls below.  Either flag below implies it.
 *   MBOTS_TRAJ_REC_OBS    each push also stores the row's rollout record -- the
 *                         content of mbots_pack_rollout, 64 B or 96 B with
 *                         MBOTS_FLAG_FIX_DEPTH_ALIAS -- in the ring slot
 *                         ([max_rows] contiguous records).  That part of the push
 *                         follows the step's sensor, as mbots_pack_rollout does;
 *                         the link / reward / value / world part still follows
 *                         the export of the rows only (two launches).
 *   MBOTS_TRAJ_REC_STATE  each push also stores HiddenState (16 f32: what the
 *                         learner wrote before the step, carried through the
 *                         sort, zero for a newborn) and a one-byte mask of the
 *                         Action that led into the row (bit i: Action[r][i] != 0),
 *                         +65 B, read where mbots_pack_learner reads the two
 *                         columns and behind the same waits.
 * The recorded bytes live in the same ring: clear(keep_last) still moves
 * nothing, the ghost's rows are never recorded, a truncated table is recorded
 * truncated, growths leave everything intact.  With all flags a row slot takes
 * 32 + 8 + 64 + 65 = 169 B (201 B with the real depth).
 *
 * A sequence is a maximal lifeline inside the n computed tables: it starts at
 * (t0, q0) with t0 == 0 or no predecessor (LINK < 0 or not a row of table
 * t0 - 1), follows NEXT and ends at the first row whose END != 0; rows of
 * table n - 1 belong to their sequences (the bootstrap element).  Every row of
 * every table lies in exactly one sequence.  Sequences are numbered 0 .. S - 1
 * in ascending (t0, q0) order, whatever the scheduling.
 *
 * mbots_traj_sequences(h, S_out, stream) fills SEQ_ID (the row's sequence) and
 * SEQ_POS (k = t - t0) for every row and returns S: the window's second host
 * synchronisation.  MBOTS_E_INVALID without MBOTS_TRAJ_SEQ, without a compute
 * of the tables now in the window, or under capture.  A later compute with
 * other parameters leaves the sequences valid; a push or a clear does not.
 *
 * mbots_traj_batch(h, lo, hi, out, stream) materialises sequences [lo, hi),
 * B = hi - lo, L = n of the last compute, start-aligned and time-major: element
 * k of column b is the row of table t0[b] + k.  Every pointer of `out` may be
 * NULL and is then skipped; the arrays are memory of the manager's device (host
 * memory in CPU mode), 4-byte aligned:
 *   rows       int32 [L, B]      the row in table t0[b] + k; -1 past the end
 *   t0, len, end  int32 [B]      start table, length (1..L), END code of the
 *                                last element (1, 2 or 3)
 *   obs        f32 [L, B, 69]    mbots_construct_obs of the stored record, bit
 *                                for bit (MBOTS_TRAJ_REC_OBS); 0.0 past the end
 *   reward, value, adv, ret  f32 [L, B]  the window's columns; 0.0 past the end
 *   action_in  uint8 [L, B]      the stored mask (MBOTS_TRAJ_REC_STATE); 0
 *   hidden0    f32 [B, 16]       HiddenState stored at the start row
 * No host synchronisation (when obs is asked for without both rows and t0, the
 * missing part of the index goes to a scratch buffer the window grows on demand
 * -- the caller's own array is still written --; a growth waits for the
 * device).  A field whose flag is
 * off, no mbots_traj_sequences of the tables now in the window, or stream
 * capture: MBOTS_E_INVALID; hi > S or lo > hi: MBOTS_E_RANGE.
 *
 * mbots_traj_gather(h, lo, hi, tables, n_tables, row_bytes, out, stream): the
 * same gather for the learner's own per-step tensors.  tables[t] (host array of
 * n_tables == n pointers) is [N_t, row_bytes] on the manager's device,
 * row_bytes a multiple of 4, at most 1024; out is [L, B, row_bytes], zero bytes
 * past the end.  The pointer list is uploaded, stream-ordered, to a buffer the
 * window owns.  Host waits: the index of a gather always goes to the window's
 * scratch buffer, so the first call, and every call whose L * B + B exceeds
 * what an earlier batch or gather needed, waits for the device and allocates;
 * every later call waits only until the previous gather's pointer list has
 * left its pinned staging (as mbots_render_worlds does for its list), never
 * for a step.  Errors as for mbots_traj_batch. */
enum mbots_traj_view_id {
    MBOTS_TRAJ_LINK = 0, MBOTS_TRAJ_NEXT = 1, MBOTS_TRAJ_END = 2, MBOTS_TRAJ_WORLD = 3,
    MBOTS_TRAJ_REWARD = 4, MBOTS_TRAJ_VALUE = 5, MBOTS_TRAJ_ADV = 6, MBOTS_TRAJ_RET = 7,
    MBOTS_TRAJ_SEQ_ID = 8, MBOTS_TRAJ_SEQ_POS = 9
};
#define MBOTS_TRAJ_SEQ       1u
#define MBOTS_TRAJ_REC_OBS   2u
#define MBOTS_TRAJ_REC_STATE 4u
struct mbots_traj_batch {   /* (a struct tag: the name is the call's too) */
    int32_t *rows;                         /* [L, B] */
    int32_t *t0, *len, *end;               /* [B] */
    float *obs;                            /* [L, B, 69] */
    float *reward, *value, *adv, *ret;     /* [L, B] */
    uint8_t *action_in;                    /* [L, B] */
    float *hidden0;                        /* [B, 16] */
};
#define MBOTS_TRAJ_END_NONE   0
#define MBOTS_TRAJ_END_DIED   1
#define MBOTS_TRAJ_END_RESET  2
#define MBOTS_TRAJ_END_WINDOW 3
int mbots_traj_open(mbots_handle *h, uint32_t horizon /* 2..65535 */, uint64_t max_rows);
int mbots_traj_close(mbots_handle *h);
int mbots_traj_push(mbots_handle *h, const float *value /* NULL: zeros */, void *stream);
int mbots_traj_compute(mbots_handle *h, float gamma, float lambda, float death_reward,
                       int64_t *rows_out /* [horizon], may be NULL */, uint32_t *n_out /* may be NULL */,
                       void *stream);
int mbots_traj_clear(mbots_handle *h, int32_t keep_last);
/* tables pushed since the last clear (host state) */
int mbots_traj_num_tables(mbots_handle *h, uint32_t *out);
int mbots_traj_view(mbots_handle *h, int32_t what, uint32_t t, mbots_tensor *out);
int mbots_traj_open_ex(mbots_handle *h, uint32_t horizon, uint64_t max_rows, uint32_t flags);
int mbots_traj_sequences(mbots_handle *h, uint64_t *S_out /* may be NULL */, void *stream);
int mbots_traj_batch(mbots_handle *h, uint64_t lo, uint64_t hi, const struct mbots_traj_batch *out, void *stream);
int mbots_traj_gather(mbots_handle *h, uint64_t lo, uint64_t hi, const void *const *tables, uint32_t n_tables,
                      uint32_t row_bytes, void *out, void *stream);

/* Rasteriser: top-down images of chosen worlds, as they stand after the last
 * step (or after create, load, reset-and-step, set_world_state or growth).  The
 * reference's viewer (src/gfx) is out of scope; this is the picture without the
 * window, and a per-world map tensor on the device with no host round trip.
 *
 * Image.  scale s in {1, 2, 4, 8} (else MBOTS_E_INVALID): H = 96 s rows by
 * W = 128 s columns.  Pixel (row j, column i) is one point sample of the arena
 * at px = (i + 0.5) / s, py = (j + 0.5) / s (exact in f32); row 0 is y ~ 0, no
 * vertical flip.  Its class is the first rule that matches, every product and
 * sum below one f32 rounding in the order written:
 *   1. agent: the lowest live slot a (as mbots_world_state lists them) with
 *      dx = px - x, dy = py - y, dx dx + dy dy <= 0.8464 (the sensor's disc of
 *      radius 0.92).  With (hx, hy) the agent's heading, fa = dx hx + dy hy and
 *      la = dy hx - dx hy, the pixel is a heading mark iff fa >= 0.3 and
 *      |la| <= 0.25: class MBOTS_RENDER_MARK + species - 1, else
 *      MBOTS_RENDER_BODY + species - 1.  The slot map holds a.
 *   2. food: any live package, centre (X, Y) in cells and (c, s) the sensor's
 *      cos / sin of its rotation, with |dx c + dy s| <= 1 and
 *      |dy c - dx s| <= 1: MBOTS_RENDER_FOOD.
 *   3. wall: the point lies in one of the four wall boxes (0.2 to either side
 *      of the border): MBOTS_RENDER_WALL.  Sample points come within 0.2 of the
 *      border only from scale 4 up (0.125 at scale 4, 0.25 at scale 2), so
 *      scales 1 and 2 show no wall: point sampling, not a missing feature.
 *   4. MBOTS_RENDER_FLOOR.
 * The slot map is -1 wherever rule 1 did not match.  rgb is the 12 x 3 palette
 * of mbots_render_palette indexed by class (entries 3 is unused and black),
 * except that a body's channels are scaled by its health:
 * k = 64 + 191 min(max(health, 0), 100) / 100, channel = base k / 255, both
 * divisions truncating int32.  Both execution modes give the same bytes.
 *
 * mbots_render_worlds(h, worlds, k, scale, out, stream): image i is local
 * world worlds[i] (host memory; any order, duplicates allowed; NULL: worlds
 * 0 .. k-1, nothing is uploaded).  An index >= num_worlds -- the shard ghost's
 * too, which is never rendered -- or k > num_worlds with a NULL list:
 * MBOTS_E_RANGE, nothing written.  k == 0: MBOTS_OK.  out's arrays are memory
 * of the manager's device (host memory in CPU mode), 4-byte aligned; any may
 * be NULL, not all three (MBOTS_E_INVALID).  One kernel launch covers all k
 * images; the call allocates nothing on the device except the list's staging
 * buffer, which the handle keeps and grows on demand (a call with a list waits
 * on the host only for the previous call's list upload, as mbots_reset_worlds
 * does; never for a step).  Stream-ordered like every call: it follows the
 * last step's world step, not its sensor, moves none of the step's deferred
 * columns, and a later step cannot overwrite what a queued render reads.
 * MBOTS_E_INVALID under stream capture (the list is uploaded from the host). */
#define MBOTS_RENDER_FLOOR 0
#define MBOTS_RENDER_WALL  1
#define MBOTS_RENDER_FOOD  2
#define MBOTS_RENDER_BODY  4   /* + species - 1: 4..7 */
#define MBOTS_RENDER_MARK  8   /* + species - 1: 8..11 */
typedef struct mbots_render_out {
    uint8_t *cls;    /* [k][96 s][128 s]     class codes            */
    int16_t *slot;   /* [k][96 s][128 s]     agent slot or -1       */
    uint8_t *rgb;    /* [k][96 s][128 s][3]                         */
} mbots_render_out;  /* any may be NULL, not all three; 4-byte aligned */
int mbots_render_worlds(mbots_handle *h, const uint32_t *worlds /* NULL: worlds 0..k-1 */,
                        uint32_t k, uint32_t scale, const mbots_render_out *out, void *stream);
int mbots_render_palette(uint8_t rgb[36]);

/* Acting on the device: per-species policy nets, sampling and the action write
 * in one stream-ordered call (DESIGN.md "Device actor" is the specification).
 *
 * A net (one per species 1..4) is a trunk of 1..4 Linear layers of one output
 * width H (a multiple of 16 in [16, 128]), each with an activation code --
 * 0 identity, 1 ReLU, 2 LeakyReLU(0.01), 3 Tanh, 4 ELU(1), 5 LogSigmoid --, an
 * actor head Linear(H, H), ReLU, Linear(H, 6), a critic head Linear(H, H), ReLU,
 * Linear(H, 1) and, when memory.weight is not NULL, a memory head Linear(H, 16),
 * Tanh, whose output becomes the row's HiddenState.  Its input is the row's 69
 * floats of mbots_construct_obs(prev = 0), bit for bit, followed by the row's 16
 * HiddenState floats when flags has MBOTS_POLICY_MEMORY_IN (trunk[0].in is 69
 * or 85 accordingly).  Weights are [out][in] row-major f32 (torch's layout),
 * bias [out] or NULL for zeros; the act field of the head layers is ignored.
 * Every Linear output is bias[j] followed by fmaf(x[k], W[j][k], acc) for k
 * ascending, so both execution modes and any sharding give the same bits.
 *
 * The gated memory head (DESIGN.md "Gated memory head"): with MBOTS_POLICY_GATE
 * in flags the net carries a gate head Linear(H, 16), Sigmoid beside its memory
 * head, and the row's new HiddenState is the update-gate blend of the old one
 * h (as the call read it) and the memory head's output c,
 *   z_j = sigmoid(bg_j + sum_k f_k Wg[j][k]),  h'_j = fmaf(z_j, c_j, fmaf(-z_j, h_j, h_j)),
 * f the trunk's last output: z == 1 gives c and z == 0 gives h bit for bit (a
 * -0 may come out as +0).  The sigmoid is 1 / (1 + e) for x >= 0 and e / (1 + e)
 * below, e the actor's exp(-|x|): exactly 1 from about 17 up, exactly 0 below
 * -104.  A gate needs a memory head and MBOTS_POLICY_MEMORY_IN; `gate` is read
 * only under the flag, so a caller that never sets it is untouched whatever
 * its memory holds there.  mbots_policy_eval and mbots_policy_grad ignore the
 * gate as they ignore the memory head; mbots_policy_seq_eval carries h' from
 * step to step and mbots_policy_seq_grad returns the gate's gradients.
 *
 * mbots_policy_set(h, species, net, stream): pointers are memory of the
 * manager's device (host memory in CPU mode), read in stream order on `stream`
 * (they may be freed stream-ordered after the call).  The first call for a
 * species, and a call whose widths, depth or heads (the gate among them) differ
 * from the net in place, allocates (after the device has drained) and is refused under stream
 * capture; a call with the same architecture only re-uploads on `stream` --
 * what a learner does after every optimiser step -- and is capturable.  A
 * captured mbots_policy_act pins the architecture in place at capture time.
 * MBOTS_E_INVALID for any width, depth, code or NULL weight outside the above,
 * a gate without a memory head or without MBOTS_POLICY_MEMORY_IN included.
 * mbots_policy_clear(h, species) removes the net (after the device has
 * drained; refused under capture).
 *
 * mbots_policy_act(h, flags, action_out, logp_out, value_out, out_rows, stream):
 * every table row -- mbots_num_rows(): the shard ghost's too -- of the current
 * table through its species' net; the action is sampled from the softmax of
 * the six logits (MBOTS_ACT_GREEDY: the first maximal logit) with
 *   u = u01(threefry2x32(seed, draw, global world, (species - 1) << 16 | k).x),
 * k the row's index inside its (world, species) segment, so N shards draw what
 * one device draws.  Unless MBOTS_ACT_NO_WRITE, Action receives the one-hot and
 * (nets with a memory head) HiddenState the head's output (a gated net's: the
 * blend with the row's HiddenState as the call read it), exactly as
 * mbots_write_actions(rows = mbots_num_rows()) of the same values would.  The
 * outputs (device memory, host memory in CPU mode; any may be NULL) receive
 * rows [0, min(rows, out_rows)): action int32, logp and value f32, [rows, 1].
 * The reads follow the last step's sensor as mbots_construct_obs does, the
 * writes order themselves as mbots_write_actions does; the call allocates
 * nothing, never waits for the host (the row counts are read on the device) and
 * can be captured into a graph next to mbots_step.  MBOTS_E_INVALID unless all
 * four species have a net.
 *
 * The draw counter (uint32, device memory) is read by every mbots_policy_act
 * and advanced by one after it in stream order, so a replayed graph draws
 * fresh numbers.  mbots_policy_draw(h, set, value): set != 0 stores *value
 * (stream-ordered after the manager's last call), else *value receives the
 * counter (a host wait); MBOTS_E_INVALID under capture.  It starts at 0 and is
 * not part of a checkpoint.
 *
 * mbots_policy_activation(act, x, y, n, device, stream): learner side, no
 * manager: y[i] = the actor's own activation `act` of x[i] (codes 0..5; 6 the
 * actor's exp, 7 its log, 8 the gate's sigmoid), device >= 0: device memory of that GPU on `stream`,
 * device == -1: host memory.  Both give the same bits.
 *
 * Policy groups (DESIGN.md "Policy groups"): contiguous ranges of global world
 * indices, each with four nets of its own, all acting in the one launch of
 * mbots_policy_act.  mbots_policy_groups(h, starts, n): 1..MBOTS_POLICY_MAX_GROUPS
 * ascending global world indices with starts[0] == 0; group g owns the worlds
 * [starts[g], starts[g + 1]), the last group every world from its start on
 * (n == 0 or NULL: back to the one group a manager starts with).  The indices
 * are global: a shard's worlds (world_offset) and its ghost world fall into
 * groups by their global index, and a group without a world in this manager
 * is legal.  New starts wait for the device, remove every net and are refused
 * under capture; the starts in place again change nothing.  Groups and nets
 * are not part of a checkpoint; growths, resets and loads leave them alone.
 * mbots_policy_num_groups(h, n, starts_out): *n the groups, starts_out (may
 * be NULL) their *n starts.  mbots_policy_set_group / mbots_policy_clear_group
 * are mbots_policy_set / mbots_policy_clear for one group's species (nets of
 * different groups may differ in every part of the architecture);
 * mbots_policy_set and mbots_policy_clear apply to every group.  A row's result
 * is bit for bit what a one-group manager holding the net of the row's (group,
 * species) computes for it -- the draw's key has no group in it -- and
 * mbots_policy_act asks for a net of every (group, species) whose range holds
 * one of the manager's worlds, the ghost included.  mbots_policy_segments(h,
 * out, stream): out (device memory; host memory in CPU mode) receives
 * [groups][4][2] int32, the rows [lo, hi) of every (group, species) among the
 * exported rows of the current table -- one contiguous range each, lo == hi
 * where there is none --, stream-ordered, no host wait, capturable. */
#define MBOTS_POLICY_MAX_GROUPS 64
#define MBOTS_POLICY_MEMORY_IN  1u
#define MBOTS_POLICY_GATE       2u
#define MBOTS_ACT_GREEDY    1u
#define MBOTS_ACT_NO_WRITE  2u
#define MBOTS_POLICY_MAX_TRUNK 4
struct mbots_policy_layer {
    uint32_t in, out;        /* widths */
    int32_t act;             /* activation code (trunk layers) */
    const float *weight;     /* [out][in] row-major */
    const float *bias;       /* [out], or NULL: zeros */
};
struct mbots_policy_net {
    uint32_t n_trunk;        /* 1..4 */
    struct mbots_policy_layer trunk[MBOTS_POLICY_MAX_TRUNK];
    struct mbots_policy_layer actor[2], critic[2];
    struct mbots_policy_layer memory;   /* weight NULL: no memory head */
    uint32_t flags;          /* MBOTS_POLICY_MEMORY_IN | MBOTS_POLICY_GATE */
    struct mbots_policy_layer gate;     /* read only with MBOTS_POLICY_GATE: Linear(H, 16), Sigmoid */
};
int mbots_policy_set(mbots_handle *h, uint32_t species /* 1..4 */, const struct mbots_policy_net *net, void *stream);
int mbots_policy_clear(mbots_handle *h, uint32_t species);
int mbots_policy_act(mbots_handle *h, uint32_t flags, int32_t *action_out, float *logp_out, float *value_out,
                     uint64_t out_rows, void *stream);
int mbots_policy_draw(mbots_handle *h, int32_t set, uint32_t *value);
int mbots_policy_activation(int32_t act, const float *x, float *y, uint64_t n, int32_t device, void *stream);
int mbots_policy_groups(mbots_handle *h, const uint32_t *starts, uint32_t n);      /* n == 0 / NULL: back to one group */
int mbots_policy_num_groups(mbots_handle *h, uint32_t *n, uint32_t *starts_out /* may be NULL */);
int mbots_policy_set_group(mbots_handle *h, uint32_t group, uint32_t species, const struct mbots_policy_net *net,
                           void *stream);
int mbots_policy_clear_group(mbots_handle *h, uint32_t group, uint32_t species);
int mbots_policy_segments(mbots_handle *h, int32_t *out /* [groups][4][2] */, void *stream);

/* Learning from what the actor did: a net evaluated on recorded (obs, action)
 * rows, and the gradients of its parameters (DESIGN.md "Differentiable
 * evaluate" is the specification).  Learner side, no manager: device >= 0 means
 * device memory of that GPU on `stream`, device == -1 host memory on the host
 * threads (MBOTS_CPU_THREADS); both give the same bits, whatever the grid or
 * the thread count.  `net` is what mbots_policy_set takes, with the same
 * checks; its pointers are read in stream order during the call.  The memory
 * head takes no part and receives no gradient here (mbots_policy_seq_grad
 * below trains it).
 *
 * mbots_policy_eval: obs [n][69] f32 (mbots_construct_obs rows), hidden [n][16]
 * (MBOTS_POLICY_MEMORY_IN nets; else ignored, may be NULL), action int32 [n] in
 * 0..5.  logp[r] and value[r] are bit for bit what mbots_policy_act returned
 * for that row, net and action; entropy[r] is the softmax's.  Any output may
 * be NULL.
 *
 * mbots_policy_grad: g_logp, g_value, g_entropy [n] are d loss / d output per
 * row (NULL: zeros); every non-NULL pointer of `out` receives the gradient of
 * the loss with respect to that weight ([out][in]) or bias ([out]); out->memory
 * is ignored.  n == 0 writes zeros.  The sums run in a fixed order: rows in
 * tiles of 64, tile i into accumulator i mod 256, each accumulator over its
 * rows in ascending order, the accumulators added in ascending index.  No
 * gradient is returned for obs or hidden.
 *
 * workspace: mbots_policy_grad_workspace(net, n, &bytes) bytes (enough for
 * either call of this architecture at up to n rows), 16-byte aligned, of
 * the same memory kind as the rows; its contents are scratch.  The calls
 * allocate nothing and never wait for the host, so they can be captured into a
 * graph.  An action outside 0..5 is refused on the host path (MBOTS_E_INVALID);
 * on the device it is the caller's contract (such a row takes part as if no
 * logit were its action's). */
struct mbots_policy_grad_layer {
    float *weight;           /* [out][in], or NULL: not wanted */
    float *bias;             /* [out], or NULL */
};
struct mbots_policy_grads {
    struct mbots_policy_grad_layer trunk[MBOTS_POLICY_MAX_TRUNK];
    struct mbots_policy_grad_layer actor[2], critic[2];
    struct mbots_policy_grad_layer memory;   /* mbots_policy_seq_grad only; mbots_policy_grad ignores it */
    struct mbots_policy_grad_layer gate;     /* read only when the net has MBOTS_POLICY_GATE (mbots_policy_seq_grad) */
};
int mbots_policy_grad_workspace(const struct mbots_policy_net *net, uint64_t n, uint64_t *bytes);
int mbots_policy_eval(const struct mbots_policy_net *net, const float *obs, const float *hidden,
                      const int32_t *action, uint64_t n, float *logp, float *value, float *entropy,
                      void *workspace, uint64_t workspace_bytes, int32_t device, void *stream);
int mbots_policy_grad(const struct mbots_policy_net *net, const float *obs, const float *hidden,
                      const int32_t *action, uint64_t n, const float *g_logp, const float *g_value,
                      const float *g_entropy, const struct mbots_policy_grads *out, void *workspace,
                      uint64_t workspace_bytes, int32_t device, void *stream);

/* Every group's nets in one call: the learner's half of policy groups
 * (DESIGN.md "Grouped evaluate" is the specification).  nets[groups][4] (1 <=
 * groups <= MBOTS_POLICY_MAX_GROUPS) holds the net of every (group, species);
 * an entry with n_trunk == 0 means the pair has no net.  segments
 * [groups][4][2] int32 is what mbots_policy_segments wrote -- the rows [lo, hi)
 * of every pair -- in the memory of the rows: on the device it is read by the
 * kernels only, never by the host, so a call does not wait for it.  obs,
 * hidden (needed iff any net has MBOTS_POLICY_MEMORY_IN), action and the
 * outputs are mbots_policy_eval's, [n] rows each.
 *
 * mbots_policy_eval_groups: a row inside the segment of (g, s) receives, bit
 * for bit, what mbots_policy_eval of nets[g][s] on the rows [lo, hi) alone
 * gives it; a row in no segment, or in the segment of a pair without a net,
 * receives +0.
 *
 * mbots_policy_grad_groups: out[groups][4]; every non-NULL pointer of out[g][s]
 * receives, bit for bit, what mbots_policy_grad of nets[g][s] on the rows
 * [lo, hi) and the g_* of those rows leaves there (the sums in that call's
 * order, counted from lo; zeros for an empty segment).  Entries of pairs
 * without a net are ignored; rows outside every segment take no part.
 *
 * Contract on segments: 0 <= lo <= hi <= n, pairwise disjoint.  The host path
 * refuses a violation (MBOTS_E_INVALID, naming the pair); the device reads hi
 * as min(hi, n) and lo as min(lo, hi), and disjointness is the caller's
 * contract there.  Actions as mbots_policy_eval's.
 *
 * workspace: mbots_policy_groups_workspace(nets, groups, n, &bytes) bytes,
 * 16-byte aligned, of the same memory kind as the rows; it grows with the
 * nets' weights and with 8 x min(256, ceil(n / 64)) slabs of the largest net,
 * not with 256 slabs per net.  The calls allocate nothing and never wait for
 * the host: they can be captured into a graph, and a replay reads the
 * segments then in place. */
int mbots_policy_groups_workspace(const struct mbots_policy_net *nets /* [groups][4] */, uint32_t groups, uint64_t n,
                                  uint64_t *bytes);
int mbots_policy_eval_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *segments,
                             const float *obs, const float *hidden, const int32_t *action, uint64_t n, float *logp,
                             float *value, float *entropy, void *workspace, uint64_t workspace_bytes, int32_t device,
                             void *stream);
int mbots_policy_grad_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *segments,
                             const float *obs, const float *hidden, const int32_t *action, uint64_t n,
                             const float *g_logp, const float *g_value, const float *g_entropy,
                             const struct mbots_policy_grads *out /* [groups][4] */, void *workspace,
                             uint64_t workspace_bytes, int32_t device, void *stream);

/* Training the memory head: the net run along padded sequences with the memory
 * head's output carried from step to step, and backpropagation through time
 * (DESIGN.md "Backpropagation through HiddenState" is the specification).  The
 * conventions are mbots_policy_eval's (handle-free, `device` / `stream`, the
 * same bits on both paths whatever the grid or the thread count).  `net` must
 * have a memory head and MBOTS_POLICY_MEMORY_IN; any other net is refused (it
 * has no state to carry: mbots_policy_eval).
 *
 * obs [L][B][69] f32, action int32 [L][B], length int32 [B] with 0 <=
 * length[b] <= L, hidden0 [B][16] f32: what mbots_traj_batch hands out, for one
 * species' columns.  Element (k, b) is present iff k < length[b].  Sequence b
 * is evaluated for k ascending on obs[k][b] | h_k, h_0 = hidden0[b], h_{k+1}
 * the memory head's output: on unchanged parameters logp[k][b], value[k][b]
 * and h_k are bit for bit what mbots_policy_act produced along that lifeline.
 *
 * mbots_policy_seq_eval: logp, value, entropy [L][B] and hidden [L][B][16] (the
 * h_k each present element was evaluated with); +0 at absent elements; any may
 * be NULL.
 *
 * mbots_policy_seq_grad: g_* [L][B] as mbots_policy_grad's (absent elements
 * are not read); every non-NULL pointer of `out`, out->memory included,
 * receives its gradient, backpropagated through h (dh past a sequence's last
 * step is +0).  obs and hidden0 receive none.  The sums run in a fixed order:
 * sequences in tiles of 64, tile i into accumulator i mod 256, an accumulator
 * over its tiles ascending, inside a tile k from the tile's largest length - 1
 * down to 0, inside a (tile, k) the 64 sequences ascending, the accumulators
 * added in ascending index.  With L == 1 and every length 1 the outputs and
 * the trunk / actor / critic gradients are mbots_policy_grad's bits.  B == 0
 * or L == 0 writes zeros.
 *
 * A gated net (MBOTS_POLICY_GATE): h_{k+1} is the blend above of h_k and the
 * memory head's output, and the pass back through time runs, per element and
 * HiddenState float, with z the gate's and c the memory head's output and dh
 * the carried d loss / d h_{k+1},
 *   d mem_pre  = (dh z) (1 - c^2),
 *   d gate_pre = (dh (c - h_k)) (z (1 - z)),
 *   dh_k       = dh (1 - z) + sum_j d0[j] W0[j][69 + .],
 * the two heads' input gradients joining the actor's and the critic's as
 * ((actor + critic) + memory) + gate.  out->gate receives the gate head's
 * gradients, summed in the order above (their accumulators follow the memory
 * head's, and the workspace grows by them).  With z exactly 1 the gate's
 * gradients and the direct dh term are zeros and every other gradient equals
 * the ungated net's as a value; with z exactly 0 d mem_pre is zero.
 *
 * workspace: mbots_policy_seq_workspace(net, L, B, &bytes) bytes, as above.
 * The calls allocate nothing and never wait for the host.  A length outside
 * [0, L] or a present action outside 0..5 is refused on the host path
 * (MBOTS_E_INVALID); on the device both are the caller's contract (a length is
 * read as clamped to [0, L]). */
int mbots_policy_seq_workspace(const struct mbots_policy_net *net, uint32_t L, uint64_t B, uint64_t *bytes);
int mbots_policy_seq_eval(const struct mbots_policy_net *net, const float *obs, const int32_t *action,
                          const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, float *logp,
                          float *value, float *entropy, float *hidden, void *workspace, uint64_t workspace_bytes,
                          int32_t device, void *stream);
int mbots_policy_seq_grad(const struct mbots_policy_net *net, const float *obs, const int32_t *action,
                          const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, const float *g_logp,
                          const float *g_value, const float *g_entropy, const struct mbots_policy_grads *out,
                          void *workspace, uint64_t workspace_bytes, int32_t device, void *stream);

/* Every group's recurrent nets in one call: mbots_policy_seq_eval / _grad for
 * policy groups (DESIGN.md "Grouped evaluate_sequences" is the specification).
 * The conventions are mbots_policy_eval_groups': `device` / `stream`,
 * nets[groups][4] with n_trunk == 0 for a pair without a net, out[groups][4].
 * Every net present must have a memory head and MBOTS_POLICY_MEMORY_IN; any
 * other is refused, naming the pair (mbots_policy_eval_groups evaluates those).
 * obs, action, length, hidden0, the outputs and g_* are mbots_policy_seq_eval's,
 * the whole batch of B columns; nothing is copied out of it.
 *
 * mbots_policy_seq_order: net_id int32 [B], entry b the column's 4 * group +
 * (species - 1); any value outside [0, 4 * groups) means no net.  Writes order
 * int32 [B] and segments int32 [groups][4][2]: order[lo .. hi) of pair (g, s)
 * holds exactly the columns with net_id == 4 g + s, ascending; the segments lie
 * in ascending 4 g + s from position 0; order past the last segment is -1.  A
 * stable counting sort: on the device three launches that use no atomic, never
 * wait for the host and can be captured; workspace (device path only; NULL is
 * fine on the host) MBOTS_POLICY_SEQ_ORDER_WORKSPACE(B) bytes, 4-byte aligned.
 *
 * Position p of segment (g, s), lo <= p < hi, stands for column order[p].
 * mbots_policy_seq_eval_groups: column order[p] receives, bit for bit, what
 * mbots_policy_seq_eval of nets[g][s] on the columns order[lo .. hi) alone gives
 * it; a column named by no evaluated segment, or by the segment of a pair
 * without a net, receives +0 at every step.
 *
 * mbots_policy_seq_grad_groups: every non-NULL pointer of out[g][s],
 * out[g][s].memory included, receives bit for bit what mbots_policy_seq_grad of
 * nets[g][s] on those columns and their g_* leaves there: the sums in that
 * call's order, counted in positions from lo (tiles of 64 positions, tile i
 * into accumulator i mod 256); zeros for an empty segment.
 *
 * Contract: 0 <= lo <= hi <= B, segments pairwise disjoint, every order[p] of
 * an evaluated segment in [0, B) and no column twice, lengths in [0, L],
 * present actions in 0..5.  The host path refuses each violation
 * (MBOTS_E_INVALID, naming the pair).  The device reads hi as min(hi, B) and lo
 * as min(lo, hi), a length as clamped to [0, L], and an order entry outside
 * [0, B) as a column of length 0 that is neither read nor written; duplicates
 * and overlaps are the caller's contract there.
 *
 * workspace: mbots_policy_seq_groups_workspace(nets, groups, L, B, &bytes)
 * bytes, 16-byte aligned, of the rows' memory kind; it grows with the nets'
 * weights and with 8 x min(256, ceil(B / 64)) slabs, stashes and [L][64][16] h
 * stores, not with 256 slabs per net.  The calls allocate nothing and never
 * wait for the host: they can be captured into a graph, and a replay reads
 * order and segments as they are then. */
#define MBOTS_POLICY_SEQ_ORDER_WORKSPACE(B) (((((uint64_t)(B)) + 1023u) / 1024u) * 1024u + 256u)
int mbots_policy_seq_order(const int32_t *net_id, uint64_t B, uint32_t groups, int32_t *order, int32_t *segments,
                           void *workspace, uint64_t workspace_bytes, int32_t device, void *stream);
int mbots_policy_seq_groups_workspace(const struct mbots_policy_net *nets /* [groups][4] */, uint32_t groups, uint32_t L,
                                      uint64_t B, uint64_t *bytes);
int mbots_policy_seq_eval_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *order,
                                 const int32_t *segments, const float *obs, const int32_t *action,
                                 const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, float *logp,
                                 float *value, float *entropy, float *hidden, void *workspace, uint64_t workspace_bytes,
                                 int32_t device, void *stream);
int mbots_policy_seq_grad_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *order,
                                 const int32_t *segments, const float *obs, const int32_t *action,
                                 const int32_t *length, const float *hidden0, uint32_t L, uint64_t B,
                                 const float *g_logp, const float *g_value, const float *g_entropy,
                                 const struct mbots_policy_grads *out /* [groups][4] */, void *workspace,
                                 uint64_t workspace_bytes, int32_t device, void *stream);

/* The update on the device: the A2C loss of recorded rows and one Adam step
 * over every net's parameters (DESIGN.md "Device learner step" is the
 * specification).  The conventions are mbots_policy_eval's: handle-free,
 * `device` >= 0 device memory on `stream`, -1 host memory; both give the same
 * bits, whatever the grid; the calls allocate nothing, never wait for the host
 * and can be captured into a graph.  Every operation written below is one
 * correctly rounded f32 operation, in the written order, never fused.
 *
 * mbots_policy_group_rows: rows[g] += sum over the four species of hi - lo of
 * segments[g] (int32 [groups][4][2], what mbots_policy_segments wrote, in the
 * memory of `rows`; on the device read by the kernel only).  The caller zeroes
 * rows (int64 [groups]) and calls it once per table of an update.  The host
 * path refuses lo < 0 or lo > hi; the device counts such a segment as empty.
 *
 * mbots_policy_a2c_loss: logp, value, entropy (the evaluate's outputs), adv,
 * ret [n] f32; end int32 [n], the window's END column, or NULL: every row is
 * kept; segments as above, with the contract of mbots_policy_eval_groups (the
 * host refuses a violation, the device clamps); rows int64 [groups], every
 * group's row total over the whole update.  For row r of a segment of group g:
 *     w         = keep_r * scale_g    keep_r 0 iff end[r] == MBOTS_TRAJ_END_RESET,
 *                                     else 1; scale_g = 1.0f / (float)rows[g],
 *                                     0 when rows[g] == 0
 *     g_logp    = (-adv) * w
 *     d         = value - ret
 *     g_value   = ((2 * value_coef) * d) * w
 *     g_entropy = (-entropy_coef) * w
 *     per_row   = (((-adv) * logp + value_coef * (d * d)) - entropy_coef * entropy) * w
 * Rows in no segment receive +0 in g_logp, g_value, g_entropy and take no part
 * in loss.  loss[g] (f64 [groups]) += the group's per_row values in a fixed
 * order: per species segment, row i counted from lo into f64 accumulator
 * i mod 256 in ascending i; the 256 accumulators added in ascending index to
 * +0; the four species' sums added in ascending species to +0; that sum added
 * to loss[g].  Any of the four outputs may be NULL.
 *
 * mbots_policy_adam: `tensors` (host memory, read during the call) describes
 * `count` parameter tensors: param, grad, m, v of n floats in the memory kind
 * of the call and the tensor's group < groups (<= MBOTS_POLICY_MAX_GROUPS);
 * n == 0 entries are passed over.  state [groups] in that memory starts as
 * {0, 1.0f, 1.0f}.  rows int64 [groups] in that memory, or NULL: a group with
 * rows[g] == 0 is left untouched entirely -- param, m, v and state.  Else,
 * with om1 = 1 - beta1 and om2 = 1 - beta2 computed once on the host:
 *     b1t' = b1t * beta1;  b2t' = b2t * beta2;  c1 = 1 - b1t';  c2 = 1 - b2t'
 *     m'   = beta1 * m + om1 * g
 *     v'   = beta2 * v + (om2 * g) * g
 *     p'   = p - (lr * (m' / c1)) / (sqrtf(v' / c2) + eps)
 * for every element, and then state[g] = {t + 1, b1t', b2t'}: the state is
 * advanced by a trailing launch, after every element has read it.  Tensors
 * must not overlap.  m and v 16-byte aligned let the kernel use 16-byte
 * accesses where param and grad are aligned too; any alignment of 4 works. */
struct mbots_policy_adam_tensor {
    float *param;
    const float *grad;
    float *m, *v;
    uint64_t n;
    uint32_t group;
};
struct mbots_policy_adam_state {
    uint32_t t;              /* steps taken */
    float b1t, b2t;          /* beta1^t, beta2^t as running f32 products */
};
int mbots_policy_group_rows(const int32_t *segments, uint32_t groups, int64_t *rows, int32_t device, void *stream);
int mbots_policy_a2c_loss(const float *logp, const float *value, const float *entropy, const float *adv,
                          const float *ret, const int32_t *end, uint64_t n, const int32_t *segments, uint32_t groups,
                          const int64_t *rows, float value_coef, float entropy_coef, float *g_logp, float *g_value,
                          float *g_entropy, double *loss, int32_t device, void *stream);
int mbots_policy_adam(const struct mbots_policy_adam_tensor *tensors, uint64_t count,
                      struct mbots_policy_adam_state *state, uint32_t groups, const int64_t *rows, float lr,
                      float beta1, float beta2, float eps, int32_t device, void *stream);

/* The recurrent update on the device: the same for the padded [L, B] sequence
 * batches of mbots_traj_batch, and Adam with per-group gradient clipping and
 * decoupled weight decay.  Conventions and rounding as above.
 *
 * Kept elements.  len, t0, end: int32 [B], the batch's columns; order int32
 * [B] and segments int32 [groups][4][2] as mbots_policy_seq_order wrote them
 * (positions lo..hi of pair (g, s) name the columns order[p]), with the
 * contract of mbots_policy_seq_eval_groups: the host path refuses a segment
 * outside [0, B], overlapping segments, an order entry outside [0, B) or one
 * named twice, and names the pair; the device clamps the bounds, and an entry
 * outside [0, B) is a column of length 0.  Element (k, b) is kept iff
 *     k < len[b]  and  (last_table < 0 or t0[b] + k < last_table)  and
 *     not (end[b] == MBOTS_TRAJ_END_RESET and k == len[b] - 1)
 * (a learner passes horizon - 1, the table that only bootstraps).  What is
 * dropped is a suffix of the column, so the kept elements are k < kept(b),
 *     kept(b) = m - (end[b] == MBOTS_TRAJ_END_RESET and m == len[b] ? 1 : 0),
 *     m = len[b] if last_table < 0 else min(len[b], max(last_table - t0[b], 0)),
 * and 0 where len[b] <= 0.
 *
 * mbots_policy_seq_group_rows: rows[g] (int64 [groups], zeroed by the caller)
 * += kept(b) over the columns of group g's four segments.
 *
 * mbots_policy_seq_a2c_loss: logp, value, entropy, adv, ret f32 [L][B]; rows
 * the groups' kept totals of the whole update.  A group with rows[g] == 0 is
 * passed over.  Else every kept element of a column of a segment of group g
 * takes mbots_policy_a2c_loss's formulas with w = 1.0f / (float)rows[g] at
 * address k * B + b; every other element of g_logp, g_value, g_entropy
 * receives +0 and takes no part in loss.  loss[g] (f64 [groups]) += the kept
 * per_row values in a fixed order: per species segment, position i = p - lo
 * into f64 accumulator i mod 256, in ascending i and within a column in
 * ascending k; the 256 accumulators added in ascending index to +0; the four
 * species' sums added in ascending species to +0; that sum added to loss[g].
 * Any of the four outputs may be NULL.  The host path also refuses a named
 * column's len outside [0, L]; the device reads it as min(len, L).
 *
 * mbots_policy_adam_clip: mbots_policy_adam's tensors, state and rows, and
 *   - the squared gradient norm of every group in f64: per chunk of 1024
 *     elements of a tensor, 256 accumulators a_j = ((x_4j^2 + x_4j+1^2) +
 *     x_4j+2^2) + x_4j+3^2 of the exact squares (double)g * (double)g, absent
 *     elements +0, folded as a tree a_i = a_i + a_{i+h} for i < h, h = 128, 64,
 *     .., 1; a tensor's chunks added in ascending order to +0; the group's
 *     tensors with n > 0 added in descriptor order to +0;
 *   - nrm = (float)sqrt(that) with the f64 sqrt, grad_norm[g] = nrm (f32
 *     [groups], may be NULL; written for every group);
 *   - coef = max_norm / (nrm + 1e-6f), and 1.0f where that is not < 1 or where
 *     max_norm is not a positive finite number (no clipping);
 *   - a group whose squared norm is inf or NaN is left untouched entirely, as
 *     one with rows[g] == 0;
 *   - per element gc = g * coef (when clipping), p1 = p - lw * p with lw = lr *
 *     weight_decay rounded once on the host (when weight_decay != 0), then
 *     mbots_policy_adam's update of (p1, gc, m, v).
 * workspace: 8-byte aligned memory of the call's kind, of at least the bytes
 * mbots_policy_adam_clip_workspace gives for the same tensors (their n) and
 * groups; its content is scratch. */
int mbots_policy_seq_group_rows(const int32_t *len, const int32_t *t0, const int32_t *end, uint64_t B,
                                const int32_t *order, const int32_t *segments, uint32_t groups, int32_t last_table,
                                int64_t *rows, int32_t device, void *stream);
int mbots_policy_seq_a2c_loss(const float *logp, const float *value, const float *entropy, const float *adv,
                              const float *ret, const int32_t *len, const int32_t *t0, const int32_t *end, uint32_t L,
                              uint64_t B, const int32_t *order, const int32_t *segments, uint32_t groups,
                              int32_t last_table, const int64_t *rows, float value_coef, float entropy_coef,
                              float *g_logp, float *g_value, float *g_entropy, double *loss, int32_t device,
                              void *stream);
int mbots_policy_adam_clip_workspace(const struct mbots_policy_adam_tensor *tensors, uint64_t count, uint32_t groups,
                                     uint64_t *bytes);
int mbots_policy_adam_clip(const struct mbots_policy_adam_tensor *tensors, uint64_t count,
                           struct mbots_policy_adam_state *state, uint32_t groups, const int64_t *rows, float lr,
                           float beta1, float beta2, float eps, float weight_decay, float max_norm, float *grad_norm,
                           void *workspace, uint64_t workspace_bytes, int32_t device, void *stream);

/* PPO on the device: the clipped surrogate and clipped value loss of recorded
 * rows, advantage normalisation and the KL early stop (DESIGN.md "PPO on the
 * device" is the specification).  Conventions and rounding as above: handle-
 * free, `device` >= 0 device memory on `stream`, -1 host memory, the same bits
 * from both whatever the grid; nothing allocates or waits for the host; the
 * calls can be captured.  segments, rows, end and (for the sequence calls) len,
 * t0, order, last_table and the kept elements are mbots_policy_a2c_loss's and
 * mbots_policy_seq_a2c_loss's, with the same host refusals and device clamps.
 *
 * Order of every sum below ("the two-level order"): element i of a (group,
 * species) segment, counted from lo, belongs to chunk i / C and to f64
 * accumulator i mod 256 of that chunk, in ascending i; a chunk's 256
 * accumulators are added in ascending index to +0; a segment's chunks in
 * ascending index to +0; the four species' sums in ascending species to +0;
 * that sum is added to the output slot.  For the row calls an element is a row
 * and C = 4096; for the sequence calls an element is a position p - lo of the
 * segment in `order`, C = 512, and the kept steps of column order[p] are added
 * in ascending k.
 *
 * mbots_policy_ppo_workspace: the bytes of `workspace` for a call over n rows
 * (or the L * B elements of a sequence batch) and `groups` groups; 8-byte
 * aligned memory of the call's kind whose content is scratch (the chunks'
 * partial sums).  A call refuses a smaller one.
 *
 * mbots_policy_adv_moments / mbots_policy_seq_adv_moments: moments (f64
 * [groups][3]) += {1, adv, adv * adv} in exact f64 over the group's kept rows --
 * those with end[r] != MBOTS_TRAJ_END_RESET (end NULL: all); the kept elements
 * of the sequence batch -- in the two-level order.  The caller zeroes moments
 * and passes every table of the update.
 *
 * mbots_policy_ppo_loss: logp, value, entropy (the evaluate's outputs),
 * old_logp, old_value (what act() returned when the rows were recorded), adv,
 * ret f32 [n].  lo_c = 1 - clip and hi_c = 1 + clip are rounded once on the
 * host; min(a, b) is b < a ? b : a and max(a, b) is b > a ? b : a, so a NaN in
 * the first argument stays.  With moments (f64 [groups][3], NULL: A = adv)
 *     n = moments[g][0], S1 = moments[g][1], S2 = moments[g][2]   (f64)
 *     mean = (float)(S1 / n)
 *     var  = (S2 - S1 * (S1 / n)) / (n - 1), 0 unless var > 0
 *     inv  = 1.0f / ((float)sqrt(var) + 1e-8f)
 *     and mean = 0, inv = 1 unless n >= 2
 * For row r of a segment of group g, w as mbots_policy_a2c_loss's:
 *     A      = (adv - mean) * inv
 *     lr     = logp - old_logp;  ratio = exp(lr)   (the device actor's exp)
 *     s1     = ratio * A
 *     rc     = min(max(ratio, lo_c), hi_c);  s2 = rc * A
 *     pol    = -min(s1, s2)
 *     g_logp = (s2 < s1 ? 0 : -s1) * w             a tie takes the unclipped branch
 *     d      = value - ret;  v1 = d * d
 *   value_clip > 0 and old_value not NULL:
 *     dv = value - old_value;  dc = min(max(dv, -value_clip), value_clip)
 *     d2 = (old_value + dc) - ret;  v2 = d2 * d2
 *     vl = v2 > v1 ? v2 : v1
 *     g_value = (value_coef * (v2 > v1 ? (dc == dv ? 2 * d2 : 0) : 2 * d)) * w
 *   else:
 *     vl = v1;  g_value = ((2 * value_coef) * d) * w
 *     g_entropy = (-entropy_coef) * w
 *     per_row   = ((pol + value_coef * vl) - entropy_coef * entropy) * w
 *     kl        = ((ratio - 1) - lr) * w
 *     clipped   = (rc != ratio ? 1 : 0) * w
 * Rows in no segment receive +0 in g_logp, g_value, g_entropy.  stats (f64
 * [groups][6]) += the sums, in the two-level order, of the f32 values
 *     [0] per_row  [1] pol * w  [2] vl * w  [3] entropy * w  [4] kl  [5] clipped
 * Any of the four outputs may be NULL.  Non-finite inputs propagate into the
 * sums; a NaN KL closes the gate below, and mbots_policy_adam_clip leaves a
 * group whose gradient norm is not finite untouched.
 * mbots_policy_seq_ppo_loss: the same for f32 [L][B] batches at address k * B +
 * b with w = 1.0f / (float)rows[g] for every kept element; a group with
 * rows[g] == 0 is passed over, stats included.
 * Refused: clip outside (0, 1), value_coef < 0, groups outside 1 ..
 * MBOTS_POLICY_MAX_GROUPS, a workspace smaller than needed.
 *
 * mbots_policy_ppo_gate: gate[g] = (gate[g] != 0 and rows[g] != 0 and
 * stats[g][4] <= target_kl) ? rows[g] : 0, for int64 [groups] gate and rows.
 * A NaN KL closes the gate; a closed gate stays closed until the caller sets
 * it again.  Passed as `rows` to mbots_policy_adam or mbots_policy_adam_clip,
 * the gate leaves a stopped group untouched as it leaves an idle one, so the
 * KL early stop of a multi-epoch update needs no read by the host. */
int mbots_policy_ppo_workspace(uint64_t n, uint32_t groups, uint64_t *bytes);
int mbots_policy_adv_moments(const float *adv, const int32_t *end, uint64_t n, const int32_t *segments,
                             uint32_t groups, double *moments, void *workspace, uint64_t workspace_bytes,
                             int32_t device, void *stream);
int mbots_policy_ppo_loss(const float *logp, const float *value, const float *entropy, const float *old_logp,
                          const float *old_value, const float *adv, const float *ret, const int32_t *end, uint64_t n,
                          const int32_t *segments, uint32_t groups, const int64_t *rows, const double *moments,
                          float clip, float value_clip, float value_coef, float entropy_coef, float *g_logp,
                          float *g_value, float *g_entropy, double *stats, void *workspace, uint64_t workspace_bytes,
                          int32_t device, void *stream);
int mbots_policy_seq_adv_moments(const float *adv, const int32_t *len, const int32_t *t0, const int32_t *end,
                                 uint32_t L, uint64_t B, const int32_t *order, const int32_t *segments,
                                 uint32_t groups, int32_t last_table, double *moments, void *workspace,
                                 uint64_t workspace_bytes, int32_t device, void *stream);
int mbots_policy_seq_ppo_loss(const float *logp, const float *value, const float *entropy, const float *old_logp,
                              const float *old_value, const float *adv, const float *ret, const int32_t *len,
                              const int32_t *t0, const int32_t *end, uint32_t L, uint64_t B, const int32_t *order,
                              const int32_t *segments, uint32_t groups, int32_t last_table, const int64_t *rows,
                              const double *moments, float clip, float value_clip, float value_coef,
                              float entropy_coef, float *g_logp, float *g_value, float *g_entropy, double *stats,
                              void *workspace, uint64_t workspace_bytes, int32_t device, void *stream);
int mbots_policy_ppo_gate(const double *stats, const int64_t *rows, uint32_t groups, double target_kl, int64_t *gate,
                          int32_t device, void *stream);

/* Stream ordering: every call that takes a stream enqueues on it after all
 * work this manager enqueued on the stream of its previous call (an event
 * hop when the two differ; not across a graph capture's boundary).  That
 * previous stream must still exist when a call on another stream is made
 * (torch's pooled streams always do). */
/* Build utilities (benchmark / test harness, not reference API):
 * identity-keyed synthetic action stream: one-hot(threefry(seed,step |
 * global_world, slot) % 6) written into the Action column of every live agent;
 * hidden state gets hash-derived floats when write_hidden != 0. */
int mbots_write_synthetic_actions(mbots_handle *h, uint32_t seed, uint32_t step,
                                  int32_t write_hidden, void *stream);
/* Make `stream` wait for this manager's outstanding work on its internal
 * stream (the last step's sensor).  Every accessor that needs the sensor rows
 * does this itself; a caller recording steps into a HIP graph (stream capture)
 * ends the captured sequence with it, so the capture has no unjoined work. */
int mbots_join(mbots_handle *h, void *stream);
/* Record `event` (a hipEvent_t, timing-enabled) on the internal stream after
 * the last step's sensor: a timing point for benchmarks that adds no wait to
 * any stream (bench.py's device span: the later of this and an event on the
 * caller's stream).  No step yet, or CPU mode: MBOTS_E_INVALID. */
int mbots_record_sensor_done(mbots_handle *h, void *event);
/* running total of agent-steps (sum over steps of live agents after the step) */
int mbots_agent_steps(mbots_handle *h, uint64_t *out);
/* births/respawns dropped because a world reached agent_capacity */
int mbots_overflow(mbots_handle *h, uint64_t *out);
/* Per-kernel device timing (bench.py roofline): when enabled, HIP events are
 * recorded on the launch stream around every kernel; mbots_kernel_times
 * synchronises and returns the summed milliseconds per kernel class
 * (index = enum mbots_timed_kernel) and the number of launches of each. */
enum mbots_timed_kernel {
    MBOTS_TK_WORLD_STEP = 0, MBOTS_TK_SCAN = 1, MBOTS_TK_EXPORT = 2,
    MBOTS_TK_SENSOR = 3, MBOTS_TK_SHIFT = 4, MBOTS_TK_ACTIONS = 5, MBOTS_TK_MOVE = 6,
    MBOTS_TK_OBS = 7, MBOTS_TK_COUNT = 8
};
int mbots_enable_kernel_timing(mbots_handle *h, int32_t enable);
int mbots_kernel_times(mbots_handle *h, double ms[MBOTS_TK_COUNT],
                       uint64_t launches[MBOTS_TK_COUNT]);
/* The step schedule the manager chose (diagnostics, no device call):
 * out[0] flags -- 1 K1-finder mode (the next K1 does not wait for the last
 * sensor), 2 fork by value, 4 join by value, 8 MBOTS_SWAP, 16 mixed capacity
 * classes (MBOTS_MIXED), 32 armed for episodes (both modes), 64 HiddenState is
 * lazy right now (owed as a row map, not stored: DESIGN.md), 128 PrevAction is
 * owed right now (the shift launched no gather: DESIGN.md); out[1] the last
 * value-wait epoch raised; out[2] how often the epochs restarted from 0;
 * out[3] steps run.  CPU mode: all 0 but the 32 of out[0] and out[3]. */
int mbots_schedule_info(mbots_handle *h, uint32_t out[4]);

const char *mbots_last_error(void);

/* Environment.
 * MBOTS_VALUE_FORK=0: the step's cross-stream hops (K1 -> the sensor's
 *   internal stream, and the sensor back to the next step) are event waits.
 *   Otherwise, from 2049 to 8192 worlds and while the host runs ahead of the
 *   device (up to 2048 the next step's K1 computes the finder slots itself and
 *   does not wait for the sensor; the fork is then an event wait),
 *   they are hipStreamWaitValue32 waits on signal words a kernel stores (about
 *   3 us instead of 7 per hop).  The runtime carries such a wait as a polling
 *   kernel on the waiting stream; a tool or mode that runs the device's
 *   kernels one at a time can dispatch that poller before its producer and
 *   never finish it, so the value waits are also off whenever one of
 *   MBOTS_SERIALISING_ENV is set (non-empty, not "0") when the manager is
 *   created: rocprofv3 counter collection, an HSA tools library, a legacy
 *   rocprof input file, or serialised kernel dispatch.
 * MBOTS_SWAP (read at mbots_create; above 8192 worlds): by default ("1") K1
 *   and K2 run on the internal stream before the sensor, with no cross-stream
 *   hop between them, and the caller's stream joins after K2 for the export
 *   rows (the sensor's chain sets the step's pace: -2 % against the forked
 *   schedule); MBOTS_SWAP=0 keeps K1 and K2 on the caller's stream and forks
 *   the sensor off after K2.
 * MBOTS_LAZY_PREV_ACTION (read at mbots_create): by default ("1") a shift
 *   that would gather Action alone launches nothing and owes PrevAction until
 *   somebody reads it (the same columns, no kernel in the headline loop);
 *   MBOTS_LAZY_PREV_ACTION=0 keeps the gather in every shift.
 * MBOTS_MIXED (read at mbots_create; agent_capacity above 128, outside the
 *   K1 finder mode): by default ("1") the 128-slot K1 and sensor run every
 *   world that fits them and the capacity class's kernels only the worlds K2
 *   lists (a world whose step could outgrow 128 slots, one with more than 128
 *   agents); MBOTS_MIXED=0 runs every world in the class's kernels (the same
 *   bits, slower).
 * MBOTS_CPU_THREADS: host threads of MBOTS_EXEC_CPU (default: the machine's
 *   hardware threads, at most 16).
 * MBOTS_EPOCH_START=<n> (read at mbots_create; a test hook): the value waits
 *   count their epochs on from n (at most 0x7FFFFFF0, where they restart
 *   from 0 after draining the device), so a short run crosses the restart. */
#define MBOTS_SERIALISING_ENV \
    { "ROCPROF_COUNTER_COLLECTION", "HSA_TOOLS_LIB", "ROCP_INPUT", "AMD_SERIALIZE_KERNEL", \
      "AMD_SERIALIZE_COPY" }

#ifdef __cplusplus
}
#endif
#endif
