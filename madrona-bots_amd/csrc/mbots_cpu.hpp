// mbots_cpu.hpp -- the CPU execution mode (ExecMode::CPU of the reference's
// Manager, BASELINE config 1: learn/env.py picks it when no GPU is present).
//
// The same world step as the HIP kernels -- identical float expressions (the
// shared host+device helpers of mbots_device.hpp / mbots_ray.hpp), identical
// state layout (SoA [world][slot] agent columns, packed per-chunk food
// records, a double-buffered species-major export table) -- run world-parallel
// on host threads.  Results are bit-identical to the HIP path.  Moves are eager
// (no deferred Prev* columns): the CPU mode is the plumbing configuration.
#pragma once

#include "../../include/mbots.h"
#include "mbots_device.hpp"
#include "mbots_traj.hpp"
#include "mbots_render.hpp"
#include "mbots_policy.hpp"

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace mbots {
namespace cpu {

// one half of the export table (types.hpp:228-252 + the raycast outputs)
struct Table {
    std::vector<int32_t> species, health, action, stats, pspecies, phealth, paction, pstats;
    std::vector<float> pos, sur, reward, hidden, ppos, psur, preward, phidden;
    std::vector<int8_t> sem, psem;
    std::vector<uint8_t> depth, pdepth;
    void resize(size_t rows);
};

class Sim {
public:
    explicit Sim(const mbots_config &cfg);

    void step();
    void shift_observations();
    void write_synthetic_actions(uint32_t seed, uint32_t step, bool write_hidden);
    int export_tensor(int32_t id, mbots_tensor *out);
    void construct_obs(bool prev, float *out, uint64_t out_rows) const;
    void sensor_index(int32_t *out) const;
    uint32_t num_agents() const { return N_; }
    // every table row: N plus the shard ghost's (which follow row N)
    uint32_t num_rows() const { return N_ + (W_ > Wx_ ? (uint32_t)n_[Wx_] : 0u); }
    uint32_t max_population() const
    {
        int32_t m = 0;
        for (int32_t v : n_) m = v > m ? v : m;
        return (uint32_t)m;
    }
    uint32_t world_offset_of(uint32_t w) const { return (uint32_t)world_off_[w]; }
    uint64_t agent_steps() const { return agent_steps_; }
    uint64_t overflow() const;
    Table &table() { return T_[tb_]; }
    // each export row's row in the table before the last step (-1: new), like
    // the HIP path's src_of (slim learner records)
    const int32_t *src_of() const { return src_of_.data(); }
    void world_state(uint32_t w, float *xy_rwrz, int32_t *sp_hp_finder, uint64_t *food,
                     uint32_t *food_rot, int32_t *n_out) const;
    uint32_t population(uint32_t w) const { return (uint32_t)n_[w]; }
    // mbots_set_world_state (arguments already checked): the live agents'
    // (x, y, rw, rz), the world's packed food records, rotations and count
    void set_world_state(uint32_t w, const float *xy_rwrz, const uint64_t *food, const uint32_t *food_rot,
                         int32_t n_food);
    uint64_t checkpoint_bytes() const;
    int save(void *dst, uint64_t bytes, std::string &err) const;
    int load(const void *src, uint64_t bytes, std::string &err);
    // mbots_grow_capacity (new_cap > the current capacity, already checked):
    // the per-slot arrays re-laid out to [W][new_cap] with the new slots zero,
    // the live table half as half 0 of new_cap rows per world, the rest kept --
    // what a fresh Sim of new_cap holds after load() of this one's save(), and
    // src_of() besides.  The vectors a host view may point into (the table
    // columns, the Done zeros, the sensor index) are not freed but retired, so
    // a view taken before still reads what it read, until release_retired().
    // MBOTS_E_NOMEM (nothing changed) when the new arrays cannot be allocated.
    int grow(uint32_t new_cap, std::string &err);
    void release_retired() { retired_.clear(); }
    // episodes (include/mbots.h "Episodes and resets"): the same operations as
    // the HIP path's on the host vectors.  reset_worlds: global indices, entries
    // outside this Sim's worlds (the shard ghost is one of them) ignored;
    // episodes null: each world's next one (arguments already checked, n > 0)
    void reset_worlds(const uint32_t *global_worlds, uint32_t n, const uint32_t *episodes);
    void set_episode_length(uint32_t steps);
    bool armed() const { return armed_; }
    // trajectory window (mbots_traj.hpp), the HIP path's launches as loops over
    // host memory: the current table into ring slot `slot` (value: N f32 or
    // null), and compute over the n pushed tables
    void traj_push(const TrajWin &w, uint32_t slot, const float *value) const;
    static void traj_compute(const TrajWin &w, const TrajParams &P, uint32_t n);
    static uint32_t traj_sequences(const TrajWin &w, uint32_t n, uint32_t max_count);   // returns S
    static void traj_batch(const TrajWin &w, const TrajBatch &o, uint32_t lo, uint64_t B, uint32_t n, float *obs);
    static void traj_gather(const int32_t *rows, const int32_t *t0, uint64_t B, uint32_t n,
                            const void *const *tables, uint32_t row_bytes, void *out);
    // rasteriser (mbots_render.hpp; arguments already checked): image i of
    // world worlds[i] (null: world i) into out's non-null arrays, the images
    // split over the host threads
    void render(const uint32_t *worlds, uint32_t k, uint32_t scale, const RenderOut &out) const;
    // device actor (mbots_policy.hpp), the HIP kernel as loops over the host
    // threads: every table row (the shard ghost's included) through the net
    // of its (group, species) -- layers held as [nt * 16][kp] rows --, sampled
    // with the draw counter's value `draw`; writes Action / HiddenState unless
    // kActNoWrite, and rows [0, out_rows) of the non-null outputs.
    // policy_segments: out [G][4][2], the exported rows of every (group, species)
    void policy_act(const PolGroups &groups, uint32_t flags, uint32_t draw, int32_t *action_out, float *logp_out,
                    float *value_out, uint64_t out_rows);
    void policy_segments(const PolGroups &groups, int32_t *out) const;
    const mbots_config &config() const { return cfg_; }

private:
    template <typename F> void for_worlds(F &&fn) const;
    void init_world(uint32_t w, uint32_t episode = 0, bool reset = false);
    void arm();
    void reset_pass();
    void world_step(uint32_t w, const Table &cur);
    void scan();
    void export_world(uint32_t w, const Table &cur, Table &nxt, bool init);
    // agents [lo, hi) of world w (hi < 0: all of them)
    void sensor_world(uint32_t w, Table &nxt, int lo = 0, int hi = -1);
    void sensor_by_agents(Table &nxt);

    mbots_config cfg_;
    uint32_t W_, Wx_, cap_, A_;   // simulated / exported worlds (W_ = Wx_ + the shard ghost)
    unsigned threads_;
    // agent state, [W][cap] (slot order = creation order, survivors compacted)
    std::vector<float> x_, y_, rw_, rz_, sur0_, sur1_;
    std::vector<int32_t> species_, health_, finder_, obsrow_;
    std::vector<uint32_t> stats_;
    // per world
    std::vector<int32_t> n_, cur_food_, scount_, row_base_, world_off_;
    std::vector<uint2> key_;
    std::vector<uint32_t> ctr_, overflow_, food_rot_;
    std::vector<uint64_t> food_;
    std::vector<float> sreward_;
    Table T_[2];
    int tb_ = 0;
    uint32_t N_ = 0;
    uint32_t totals_[5] = {};
    uint64_t agent_steps_ = 0;
    std::vector<int32_t> zeros_rows_, sensor_index_, src_of_;
    // episodes, per simulated world: the live reset flags (MBOTS_EXPORT_RESET),
    // the current episode, the steps since the last reset or creation (kept by
    // the reset pass once armed; age0_ for every world before)
    std::vector<int32_t> reset_flags_, episode_, age_;
    std::vector<int32_t> reset_mark_;   // 1: the last reset pass re-initialised the world
    bool armed_ = false;
    uint32_t ep_len_ = 0;
    uint64_t age0_ = 0;
    std::vector<std::shared_ptr<void>> retired_;   // vectors earlier growths left (grow())
};

// evaluate and its backward pass on host threads (mbots_policy.hpp; no
// simulator): `net` in the CPU mode's [nt * 16][kp] layout.  The gradient call
// fills slabs.nacc slabs ([out][in] / [out] per layer), threads splitting the
// accumulators, then adds them in ascending index into `out`.
void policy_eval(const PolNet &net, const PolEvalIO &io);
void policy_grad(const PolNet &net, const PolEvalIO &io, const PolGradSlabs &slabs, const PolGradOut &out);
// evaluate_sequences on the host threads; hws as the device's (mbots_kernels.hpp).
// cols: the batch columns the call runs, position p standing for column
// cols.idx[p] (the grouped call's segments); tiles and chains count positions.
void policy_seq_eval(const PolNet &net, const PolSeqIO &io, const PolSeqCols &cols = PolSeqCols{nullptr, 0});
void policy_seq_grad(const PolNet &net, const PolSeqIO &io, const PolGradSlabs &slabs, float *hws,
                     const PolGradOut &out, const PolSeqCols &cols = PolSeqCols{nullptr, 0});

}  // namespace cpu
}  // namespace mbots
