/*
 * mbots_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C11) of the llGuy/madrona-bots per-step simulation
 * (src/sim/sim.cpp, src/sim/sim.inl, src/sim/types.hpp, src/entry/mgr.cpp).
 * It is the parity checker for the HIP product path and the CPU baseline of
 * bench.py.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg may load it.  The product (madrona-bots_amd/) never links or calls it.
 *
 * PARITY STATUS.  The simulation part is held bitwise to the reference's own
 * compiled sim.cpp, run on the stand-in engine of oracle/refbuild/
 * (tests/test_reference_pin.py live, tests/golden/reference_*.npz recorded;
 * DESIGN.md section 7).  The engine itself (the un-vendored Madrona submodule)
 * stays the build's written spec, "parity unpinned":
 *
 *   pinned by the reference's compiled code | decided by the build's spec
 *   ----------------------------------------+-----------------------------------
 *   every expression, branch, constant and  | RNG (Threefry-2x32-20, key
 *   cast of the step and shift systems      | schedule, sampleUniform, sampleI32)
 *   RNG draw counts, the discarded draws    | quaternion arithmetic
 *   the quirks ((uint32_t)(len*2.f), the    | iteration, creation and deletion
 *   clamp order, health > 10 after +20,     | order; the observation sort
 *   hitEnemy = hitFriendly, rewards[id],    | the consume contention outcome
 *   SpeciesCount before the respawns)       | the memory behind rewards[4]
 *   initWorld, makeAgent, the Sim           | the sensor and the finder
 *   constructor's key                       | capacity; dead agents' rows (B.4),
 *   the chunk helpers, FoodPackage::consume | new rows (B.13), the first export
 *   the order of the step and shift graphs  | resets and episodes
 *
 * Boundary shapes are pinned by the reference checkpoints (obs width 69, action
 * width 6: tests/golden/).
 *
 * RESETS AND EPISODES: the oracle restates them too, written from
 * INTEGRATION.md "Episodes and resets" and the reference's key schedule
 * (sim.cpp:64-75, :1236-1240: split_i(initKey, episode, world)) and not from
 * the product's reset pass: a reset clears the world and runs the same
 * per-world constructor orc_create runs, with the episode in the key.  Pinned
 * by known answers of its own in tests/test_oracle_kat.py (positions from
 * Threefry, all-reset == fresh, one reset world == a one-world oracle, the
 * episode length, the two flag forms, the faithful reward over a reset
 * neighbour); tests/test_reset_oracle.py and the episode call sequences of
 * tests/test_parity_gpu.py / tests/test_reset_sequences_cpu.py hold both
 * execution modes of the product against it.
 */
#ifndef MBOTS_ORACLE_H
#define MBOTS_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/sim/types.hpp:13-14, :78-80; src/entry/mgr.cpp:104-113 */
#define ORC_NUM_SPECIES   4
#define ORC_HIDDEN        16
#define ORC_SENSOR        32
#define ORC_CHUNKS_X      8
#define ORC_CHUNKS_Y      6
#define ORC_NUM_CHUNKS    48
#define ORC_CHUNK_W       16
#define ORC_MAX_PKG       5
#define ORC_FOOD_CAP      30

typedef struct orc_sim orc_sim;

typedef struct {
    uint32_t num_worlds;        /* worlds held by this instance            */
    uint32_t world_offset;      /* global index of world 0 (sharding)     */
    uint32_t rand_seed;
    uint32_t init_agents;       /* initNumAgentsPerWorld                   */
    uint32_t cap;               /* per-world agent slot capacity           */
    uint32_t reward_fixed;      /* 0: faithful rewards[speciesID]; 1: [id-1] */
    uint32_t num_threads;       /* host threads for the world loops        */
} orc_config;

/* Column identifiers of the exported observation table (mgr.cpp:199-422). */
enum {
    ORC_COL_SPECIES = 0,  /* int32 [N]      */
    ORC_COL_POS,          /* f32   [N][2]   */
    ORC_COL_HEALTH,       /* int32 [N]      */
    ORC_COL_SURROUND,     /* f32   [N][2]   */
    ORC_COL_REWARD,       /* f32   [N]      */
    ORC_COL_ACTION,       /* int32 [N][6]   */
    ORC_COL_STATS,        /* int32 [N][4]   */
    ORC_COL_HIDDEN,       /* f32   [N][16]  */
    ORC_COL_SEMANTIC,     /* int8  [N][32]  */
    ORC_COL_DEPTH,        /* uint8 [N][32]  */
    ORC_NUM_COLS
};

orc_sim *orc_create(const orc_config *cfg);
void     orc_destroy(orc_sim *s);
void     orc_step(orc_sim *s);
void     orc_shift_observations(orc_sim *s);
uint32_t orc_num_agents(const orc_sim *s);
/* pointer to the current (is_prev=0) or Prev* (is_prev=1) column */
void    *orc_column(orc_sim *s, int col, int is_prev);
int32_t *orc_species_count(orc_sim *s);           /* [W][4]          */
/* per-world agent counts / world-major offsets (agentOffsetForWorld) */
void     orc_world_counts(const orc_sim *s, int32_t *counts, int32_t *offsets);
/* identity-keyed synthetic action stream: one-hot(hash(seed,step,gw,slot)%6);
 * hidden[k] = hash-derived float when write_hidden != 0 */
void     orc_write_synthetic_actions(orc_sim *s, uint32_t seed, uint32_t step,
                                     int write_hidden);
/* per-world agent slot -> export row (sensorIndexTensor in world-major order) */
void     orc_sensor_index(const orc_sim *s, int32_t *out);
uint32_t orc_overflow(const orc_sim *s);
/* debug views of the per-world slot state (tests) */
void     orc_world_state(const orc_sim *s, uint32_t w, float *xy, float *rot,
                         int32_t *species, int32_t *health, int32_t *finder,
                         int32_t *n);
/* live food packages of world w in (chunk, package) order: out[k] = (chunk,
 * x, y, 22-bit rotation); returns their count (<= 240 entries of 4) */
int32_t  orc_world_food(const orc_sim *s, uint32_t w, int32_t *out);
/* the inverse for geometry (tests place a chosen scene in front of the
 * sensor): writes ag[i].x / y / rw / rz for the world's n_agents live agents
 * (rows of 4 f32) and replaces its food by n_food packages (chunk, x, y,
 * rotation) as orc_world_food reports them, each chunk's slots filled from 0
 * in the order given; cur_food follows.  Population, species, health, finder
 * slots, RNG and the export table are untouched.  Returns 0, or -1 with
 * nothing written under the conditions of mbots_set_world_state
 * (include/mbots.h): another population, a position outside [0, 127] x
 * [0, 95], a rotation off the unit circle by more than 1e-3, more than 5
 * packages in a chunk or 30 in the world, a package outside its chunk, a
 * rotation >= 2^22 */
int      orc_set_world_state(orc_sim *s, uint32_t w, const float *xy_rwrz, uint32_t n_agents,
                             const int32_t *food, uint32_t n_food);

/* Episodes and resets (see the header comment).  At the start of orc_step,
 * per world: with flag 0 and (length 0 or episode_step < length) the world's
 * episode_step grows by one; otherwise its episode becomes flag - 2 (flag >= 2)
 * or episode + 1, the world is cleared to a not yet constructed one and
 * constructed again from threefry2x32((seed, 0), (episode, global world)),
 * episode_step = 1, flag = 0 -- and then it steps like every other world, its
 * agents' rows new (Action, HiddenState and every Prev column zero).  The
 * dropped-agent counter (orc_overflow) stays cumulative.  An oracle on which
 * none of these is called does what it did before they existed. */
/* flag the listed global worlds: 1 (episodes == NULL) or episodes[k] + 2;
 * indices outside [world_offset, world_offset + num_worlds) are ignored */
void     orc_reset_worlds(orc_sim *s, const uint32_t *global_worlds, uint32_t n,
                          const uint32_t *episodes);
void     orc_set_episode_length(orc_sim *s, uint32_t steps);       /* 0: off */
int32_t *orc_reset_flags(orc_sim *s);         /* [W] live: a test may write */
const int32_t *orc_episode(const orc_sim *s);                      /* [W]   */
const int32_t *orc_episode_step(const orc_sim *s);                 /* [W]   */

/* exposed primitives for known-answer tests */
/* one food box (centre (cx, cy), 22-bit rotation) seen from an agent at
 * (ax, ay) with heading (hx, hy): hit[k] / depth z[k] per ray (32 pixels,
 * the finder ray last) */
void     orc_probe_box(float ax, float ay, float hx, float hy, float cx, float cy,
                       uint32_t rot, uint8_t *hit, float *z);
/* the same for another agent's disc centred at (cx, cy) */
void     orc_probe_agent(float ax, float ay, float hx, float hy, float cx, float cy,
                         uint8_t *hit, float *z);
/* what each ray of a lone agent sees of the walls: sem[k] (5 wall, -1 miss)
 * and depth[k] bytes (the finder ray last: 5 / -1) */
void     orc_probe_walls(float ax, float ay, float hx, float hy, int8_t *sem, uint8_t *depth);
void     orc_threefry2x32(const uint32_t key[2], const uint32_t ctr[2],
                          uint32_t out[2]);
float    orc_sample_uniform(uint32_t bits);
int32_t  orc_sample_i32(uint32_t bits, int32_t a, int32_t b);
uint32_t orc_action_hash(uint32_t seed, uint32_t step, uint32_t gworld,
                         uint32_t slot);

#ifdef __cplusplus
}
#endif
#endif
