// mbots_manager.cpp -- host orchestration (the reference's Manager,
// src/entry/mgr.cpp) behind the C ABI declared in include/mbots.h.
//
// MI355X-first differences from the reference Manager:
//  * no runtime compilation: kernels are ahead-of-time gfx950 code objects;
//  * every launch goes on the caller's HIP stream (torch's current stream), and
//    step() does not block -- the host-side agent count is fetched lazily by an
//    async D2H copy into pinned memory plus an event (mgr.cpp:57-62 did two
//    blocking cudaMemcpy per step);
//  * all device memory is one arena sized for `num_worlds * agent_capacity`
//    rows (288 GB HBM per GPU leaves ample headroom);
//  * the species-major export table is double-buffered: a step writes the new
//    table while reading the old one (no in-place radix sort of 264-B rows).
#if defined(MB_PROBE_NO_JOIN) && !defined(MB_PROBE_BUILD)
#error "MB_PROBE_NO_JOIN gives wrong finder slots: a probe build (scripts/build_var.sh -DMB_PROBE_BUILD) only"
#endif
#include <hip/hip_ext.h>
#include "../../include/mbots.h"
#include "mbots_kernels.hpp"
#include "mbots_cpu.hpp"
#include "mbots_defer.hpp"
#include "mbots_sched.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(MBOTS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Arena {
    char *base = nullptr;
    size_t used = 0, size = 0;
    template <typename T>
    T *take(size_t count)
    {
        size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
        T *p = reinterpret_cast<T *>(base + used);
        used += bytes;
        return p;
    }
};

struct TimedPair {
    hipEvent_t a, b;
    int kind;
};

}  // namespace

struct mbots_handle {
    mbots_config cfg{};
    std::unique_ptr<mbots::cpu::Sim> cpu;   // MBOTS_EXEC_CPU: the host world step
    int device = 0;
    mbots::SimState S{};
    mbots::ObsTable T[2]{};
    Arena arena;
    int32_t *done_zeros = nullptr;    // Done column (never written, sim.cpp:74-75, B.7)
    int32_t *reset_flags = nullptr;   // WorldReset singleton per world: the live flag array
                                      // (MBOTS_EXPORT_RESET; zeros until someone writes)
    // episodes (include/mbots.h "Episodes and resets"): per simulated world, the
    // shard ghost included
    int32_t *episode = nullptr;       // the world's current episode
    int32_t *age = nullptr;           // steps since its last reset or creation (kept by the
                                      // reset pass: current once armed, or filled on export)
    bool armed = false;               // every step runs the reset pass before K1
    int32_t *reset_mark = nullptr;    // [W] 1: the last reset pass re-initialised the world (its
                                      // own allocation: a growth leaves it; the trajectory
                                      // window's push copies it)
    uint32_t ep_len = 0;              // episode length in steps (0: off)
    uint64_t age0 = 0;                // steps since creation (every world's age while unarmed)
    int32_t *flag_stage = nullptr;    // mbots_reset_worlds: pinned host / device staging of
    int32_t *flag_stage_dev = nullptr;   // one value per world, and the event after its last
    hipEvent_t ev_stage = nullptr;    // upload
    uint32_t *render_list = nullptr;      // mbots_render_worlds: pinned host / device staging of
    uint32_t *render_list_dev = nullptr;  // its world list (grown on demand), and the event
    uint32_t render_list_cap = 0;         // after its last upload
    hipEvent_t ev_render_list = nullptr;
    int32_t *sensor_index = nullptr;  // scratch for sensorIndexTensor
    uint32_t *h_totals = nullptr;     // pinned mirror of S.totals
    // the step's cross-queue ordering (mbots_sched.hpp), and the HIP objects its
    // indices name: the sensor's internal stream (forked after K2), the events
    // (ev[kTotals] also orders the host's reads of h_totals) and the signal
    // words of the value waits (null: event waits)
    mbots::sched::Schedule sched;
    hipStream_t aux = nullptr;
    hipEvent_t ev[mbots::sched::kNumEvents] = {};
    uint32_t *sig[2] = {nullptr, nullptr};
    bool sensed = false;              // a sensor has run since init (the finder slots are then
                                      // the centre ray's, before it the init's "none")
    int32_t *row_base2[2] = {nullptr, nullptr};   // row bases / sensor order of alternate
    int32_t *sorder2[2] = {nullptr, nullptr};     // steps (a sensor may still read the last
                                                  // step's while the next K2 writes)
    int32_t *obsrow_out2[2] = {nullptr, nullptr}; // K1's old-row column of alternate steps (in
                                                  // K1-finder mode the sensor reads the last
                                                  // step's while the next K1 writes)
    uint32_t ovf_reported = 0;        // capacity drops reported so far (MBOTS_W_CAPACITY)
    // the deferred columns of the two table halves, the current half and the
    // step parity (mbots_defer.hpp)
    mbots::defer::Deferred defer;
    bool pa_on = true;                // MBOTS_LAZY_PREV_ACTION (read at create)
    int32_t *hid_map2[2] = {nullptr, nullptr};   // lazy HiddenState's row maps of alternate steps (by parity)
    int32_t *src_of2[2] = {nullptr, nullptr};   // src_of of alternate steps (by parity): K3a
                                                // writes this step's, S.src_of names it
    uint32_t *lazy_rows = nullptr;    // device words K2 stores the table's rows into: [parity]
                                      // for lazy HiddenState, [2 + parity] for owed PrevAction
                                      // ([4]: the word a lazy shift's own launch stores)
    bool totals_ok = false;           // h_totals holds the last step's counts (synchronised)
    bool maxpop_stale = false;        // no K2 since a checkpoint load: the tile maxima are old
    uint64_t steps = 0;               // steps run
    bool timing = false;
    std::vector<TimedPair> pending;
    std::vector<hipEvent_t> pool;
    double acc_ms[MBOTS_TK_COUNT] = {};
    uint64_t acc_n[MBOTS_TK_COUNT] = {};
    bool auto_cap = false;            // mbots_set_auto_capacity: mbots_step grows before it could overflow
    // the trajectory window (include/mbots.h "Trajectory window"): storage of its
    // own (one allocation, device or host), so growths leave it alone
    struct Traj {
        bool open = false;
        mbots::TrajWin w{};
        void *mem = nullptr;
        uint32_t n = 0;               // tables pushed
        uint32_t known = 0;           // tables whose row count the host holds (rows)
        bool computed = false;        // next / end / adv / ret are those of the n tables
        std::vector<int64_t> rows;    // N_t of table t < known
        uint32_t *h_count = nullptr;  // pinned staging of w.count (HIP mode)
        // the opt-in parts (mbots_traj_open_ex)
        uint32_t flags = 0;
        bool seq_valid = false;       // SEQ_ID / SEQ_POS are those of the computed tables
        uint32_t S = 0;               // their sequences
        uint32_t mx = 0;              // the largest N_t of the computed tables
        uint32_t *h_S = nullptr;      // pinned staging of S
        int32_t *idx = nullptr;       // index scratch of a batch / gather ([L][B] rows, [B] t0) when the
        uint64_t idx_cap = 0;         // caller gives no arrays of its own: grown on demand (int32 entries)
        const void **tabs = nullptr;  // mbots_traj_gather's pointer list: the window's device buffer
        const void **h_tabs = nullptr;   // ([horizon]), its pinned staging and the event after the
        hipEvent_t ev_tabs = nullptr;    // last upload
    } traj;
    // the device actor (include/mbots.h "Acting on the device"): per (group,
    // species) one allocation of its own holding the uploaded layers (fragment
    // order in HIP mode, padded rows in CPU mode), so growths leave it alone
    struct Policy {
        std::vector<uint32_t> starts = std::vector<uint32_t>(1, 0u);   // the groups' first global worlds
        std::vector<mbots::PolNet> nets = std::vector<mbots::PolNet>(mbots::kNumSpecies);   // [G][4]
        std::vector<float *> mem = std::vector<float *>(mbots::kNumSpecies, nullptr);      // [G][4]
        mbots::PolNet *table = nullptr;   // HIP mode, once there were groups: the device's copy of
                                          // `nets`, [MBOTS_POLICY_MAX_GROUPS][4] (a captured act reads it in place)
        uint32_t groups() const { return (uint32_t)starts.size(); }
        uint32_t *draw = nullptr;     // the device's draw counter (HIP mode)
        uint32_t draw_host = 0;       // CPU mode's
    } pol;
    std::vector<char *> retired;      // arenas earlier growths left (views taken then still read
                                      // them): freed by mbots_release_retired / mbots_destroy
};

namespace {

#ifndef MB_FINDER_PSEM_BY_SENSOR
#define MB_FINDER_PSEM_BY_SENSOR 1   // K1-finder mode: the sensor moves the prev-sensor rows itself
#endif
bool env_set(const char *name)
{
    const char *v = std::getenv(name);
    return v && *v && std::strcmp(v, "0") != 0;
}
// the environment's part of the schedule's choice (the list and the switches
// are documented in include/mbots.h, "Environment")
mbots::sched::Knobs sched_knobs()
{
    mbots::sched::Knobs k;
    const char *o = std::getenv("MBOTS_VALUE_FORK");
    if (o && std::strcmp(o, "0") == 0) k.value_waits_safe = false;
    static const char *const kSerialising[] = MBOTS_SERIALISING_ENV;
    for (const char *name : kSerialising)
        if (env_set(name)) k.value_waits_safe = false;
    const char *e = std::getenv("MBOTS_SWAP");
    if (e && *e) k.swap = e[0] == '1' ? 1 : 0;
    return k;
}

bool mixed_wanted()
{
    const char *e = std::getenv("MBOTS_MIXED");
    return !(e && *e == '0');
}

hipEvent_t get_event(mbots_handle *h)
{
    if (!h->pool.empty()) {
        hipEvent_t e = h->pool.back();
        h->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

template <typename F>
int timed(mbots_handle *h, int kind, hipStream_t st, F &&launch)
{
    TimedPair tp{nullptr, nullptr, kind};
    if (h->timing) {
        tp.a = get_event(h);
        tp.b = get_event(h);
        HIP_TRY(hipEventRecord(tp.a, st));
    }
    HIP_TRY(launch());
    if (h->timing) {
        HIP_TRY(hipEventRecord(tp.b, st));
        h->pending.push_back(tp);
    }
    return MBOTS_OK;
}

void fill_table(mbots::ObsTable &t, Arena &a, size_t rows)
{
    using namespace mbots;
    t.species = a.take<int32_t>(rows);
    t.pos = a.take<float>(rows * 2);
    t.health = a.take<int32_t>(rows);
    t.sur = a.take<float>(rows * 2);
    t.reward = a.take<float>(rows);
    t.action = a.take<int32_t>(rows * 6);
    t.stats = a.take<int32_t>(rows * 4);
    t.hidden = a.take<float>(rows * kHidden);
    t.sem = a.take<int8_t>(rows * kSensor);
    t.depth = a.take<uint8_t>(rows * kSensor);
    t.pspecies = a.take<int32_t>(rows);
    t.ppos = a.take<float>(rows * 2);
    t.phealth = a.take<int32_t>(rows);
    t.psur = a.take<float>(rows * 2);
    t.preward = a.take<float>(rows);
    t.paction = a.take<int32_t>(rows * 6);
    t.pstats = a.take<int32_t>(rows * 4);
    t.phidden = a.take<float>(rows * kHidden);
    t.psem = a.take<int8_t>(rows * kSensor);
    t.pdepth = a.take<uint8_t>(rows * kSensor);
}

size_t layout(mbots_handle *h, Arena &a)
{
    using namespace mbots;
    const size_t W = h->S.W, cap = h->cfg.agent_capacity, rows = W * cap;
    SimState &S = h->S;
    S.x = a.take<float>(rows);
    S.y = a.take<float>(rows);
    S.rw = a.take<float>(rows);
    S.rz = a.take<float>(rows);
    S.species = a.take<int32_t>(rows);
    S.health = a.take<int32_t>(rows);
    S.finder = a.take<int32_t>(rows);
    S.obsrow = a.take<int32_t>(rows);
    S.sur0 = a.take<float>(rows);
    S.sur1 = a.take<float>(rows);
    S.stats = a.take<uint32_t>(rows);
    S.n = a.take<int32_t>(W);
    S.ctr = a.take<uint32_t>(W);
    S.key = a.take<uint2>(W);
    S.food = a.take<uint64_t>(W * kNumChunks);
    S.food_rot = a.take<uint32_t>(W * kNumPkg);
    S.cur_food = a.take<int32_t>(W);
    S.sreward = a.take<float>(W * kNumSpecies);
    S.scount = a.take<int32_t>(W * kNumSpecies);
    h->row_base2[0] = a.take<int32_t>(W * kNumSpecies);
    h->row_base2[1] = a.take<int32_t>(W * kNumSpecies);
    S.row_base = h->row_base2[0];
    S.world_off = a.take<int32_t>(W);
    h->src_of2[0] = a.take<int32_t>(rows);
    h->src_of2[1] = a.take<int32_t>(rows);
    S.src_of = h->src_of2[0];
    h->hid_map2[0] = a.take<int32_t>(rows);
    h->hid_map2[1] = a.take<int32_t>(rows);
    h->lazy_rows = a.take<uint32_t>(5);
    S.map_in = nullptr;
    S.map_out = nullptr;
    S.rows_out = nullptr;
    S.overflow = a.take<uint32_t>(W);
    S.fork_ctr = a.take<uint32_t>(1);
    S.totals = a.take<uint32_t>(8);
    S.ntiles = scan_tiles((uint32_t)W);
    S.tiles = a.take<int32_t>((size_t)2 * S.ntiles * kTileBuckets * 5);
    S.agent_steps = a.take<unsigned long long>(1);
    S.raytab = a.take<float4>(36);
    S.big_k1 = a.take<int32_t>(2 * W);   // mixed capacity classes (K2's lists)
    S.big_s = a.take<int32_t>(2 * W);
    S.big_cnt = a.take<uint32_t>(4);
    h->sorder2[0] = h->sorder2[1] = nullptr;
    if (sensor_order_used((uint32_t)W)) {
        h->sorder2[0] = a.take<int32_t>(W);
        h->sorder2[1] = a.take<int32_t>(W);
    }
    S.sorder = h->sorder2[0];
    S.x_out = a.take<float>(rows);
    S.y_out = a.take<float>(rows);
    S.rw_out = a.take<float>(rows);
    S.rz_out = a.take<float>(rows);
    S.species_out = a.take<int32_t>(rows);
    h->obsrow_out2[0] = a.take<int32_t>(rows);
    h->obsrow_out2[1] = a.take<int32_t>(rows);
    S.obsrow_out = h->obsrow_out2[0];
    S.n_out = a.take<int32_t>(W);
    S.food_out = a.take<uint64_t>(W * kNumChunks);
    fill_table(h->T[0], a, rows);
    fill_table(h->T[1], a, rows);
    h->done_zeros = a.take<int32_t>(rows);
    h->reset_flags = a.take<int32_t>(W);
    h->episode = a.take<int32_t>(W);
    h->age = a.take<int32_t>(W);
    h->sensor_index = a.take<int32_t>(rows);
    return a.used;
}

hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// table half `half` as its readers see it: an aliased current Action /
// HiddenState column read from its Prev column
mbots::ObsTable src_view(const mbots_handle *h, int half)
{
    mbots::ObsTable t = h->T[half];
    if (h->defer.action_aliased(half)) t.action = t.paction;
    if (h->defer.hidden_aliased(half)) t.hidden = t.phidden;
    return t;
}

hipStream_t last_stream(const mbots_handle *h)
{
    return static_cast<hipStream_t>(const_cast<void *>(h->sched.last_stream));
}

// The executor of one call into the manager on stream `st`: the runtime calls
// of the schedule's rules (mbots_sched.hpp) and the device work of the deferred
// columns' rules (mbots_defer.hpp: each operation on the stream the caller uses
// next, timed as a move).  The capture `st` is recorded into is asked of the
// runtime once per call
int sync_totals(mbots_handle *h);
struct Exec {
    mbots_handle *h;
    hipStream_t st;
    bool cap_known = false;
    unsigned long long cap_id = 0;
    int cap_rc = MBOTS_OK;

    static int query_capture(hipStream_t s, unsigned long long &id)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        unsigned long long cid = 0;
        id = 0;
        const hipError_t e = hipStreamGetCaptureInfo(s, &cs, &cid);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MBOTS_E_HIP, std::string("hipStreamGetCaptureInfo: ") + hipGetErrorString(e));
        }
        if (cs == hipStreamCaptureStatusActive) id = cid;
        return MBOTS_OK;
    }
    hipStream_t queue(int q) const
    {
        switch (q) {
        case mbots::sched::kSensor: return h->aux;
        case mbots::sched::kLast: return last_stream(h);
        case mbots::sched::kCapture: return static_cast<hipStream_t>(const_cast<void *>(h->sched.cap_stream));
        default: return st;
        }
    }
    const void *caller() const { return st; }
    int capture_of(int q, unsigned long long &id)
    {
        const hipStream_t s = queue(q);
        if (s != st || q == mbots::sched::kCapture) return query_capture(s, id);
        if (!cap_known) {
            cap_rc = query_capture(st, cap_id);
            cap_known = true;
        }
        id = cap_id;
        return cap_rc;
    }
    bool capturing()
    {
        unsigned long long id = 0;
        return capture_of(mbots::sched::kCaller, id) == MBOTS_OK && id != 0;
    }
    int record(int ev, int q)
    {
        HIP_TRY(hipEventRecord(h->ev[ev], queue(q)));
        return MBOTS_OK;
    }
    int wait_event(int q, int ev)
    {
        HIP_TRY(hipStreamWaitEvent(queue(q), h->ev[ev], 0));
        return MBOTS_OK;
    }
    int wait_value(int q, int sig, uint32_t epoch)
    {
        HIP_TRY(hipStreamWaitValue32(queue(q), h->sig[sig], epoch, hipStreamWaitValueGte, 0xFFFFFFFFu));
        return MBOTS_OK;
    }
    int raise_join(uint32_t epoch)
    {
        HIP_TRY(mbots::launch_raise_flag(h->sig[mbots::sched::kJoin], epoch, h->aux));
        return MBOTS_OK;
    }
    bool pending(int ev)
    {
        const bool busy = hipEventQuery(h->ev[ev]) == hipErrorNotReady;
        (void)hipGetLastError();   // (hipEventQuery reports "not ready" as an error)
        return busy;
    }
    int drain_and_zero()
    {
        HIP_TRY(hipDeviceSynchronize());
        for (uint32_t *p : h->sig)
            if (p) HIP_TRY(hipMemset(p, 0, 8));
        HIP_TRY(hipDeviceSynchronize());
        return MBOTS_OK;
    }
    int refuse(mbots::sched::Refusal why, uint64_t n)
    {
        switch (why) {
        case mbots::sched::kCaptureElsewhere:
            return fail(MBOTS_E_INVALID, "a graph capture of this manager's steps is still recording on another "
                                         "stream: call the manager on the capturing stream, or after the "
                                         "capture has ended");
        case mbots::sched::kOddJoin:
            return fail(MBOTS_E_INVALID, "a captured sequence must hold an even number of steps (" +
                                             std::to_string(n) + " recorded)");
        default:
            return fail(MBOTS_E_INVALID, "the last graph capture recorded an odd number of steps, so the manager's "
                                         "table halves no longer follow the device; capture an even number of steps "
                                         "(ending with join()) and create a new manager");
        }
    }

    template <class F> int run(int kind, F &&launch)
    {
        HIP_TRY(hipSetDevice(h->device));
        return timed(h, kind, st, launch);
    }
    int move(int part, bool six_lazy)
    {
        const int tb = h->defer.tb;
        const mbots::ObsTable src = part == mbots::kMoveAH ? src_view(h, tb ^ 1) : h->T[tb ^ 1];
        return run(MBOTS_TK_MOVE, [&] { return mbots::launch_move(h->S, src, h->T[tb], six_lazy ? 1 : 0, part, st); });
    }
    int move_shift(int word)
    {
        const int tb = h->defer.tb;
        const mbots::ObsTable src = src_view(h, tb ^ 1);
        return run(MBOTS_TK_SHIFT, [&] {
            return mbots::launch_move(h->S, src, h->T[tb], 0, mbots::kMoveAHShift, st,
                                      word >= 0 ? h->lazy_rows + word : nullptr);
        });
    }
    int shift(bool rest)
    {
        return run(rest ? MBOTS_TK_MOVE : MBOTS_TK_SHIFT, [&] {
            return mbots::launch_shift(h->S, h->T[h->defer.tb], rest ? mbots::kShiftRest : mbots::kShiftEager, st);
        });
    }
    int gather_hidden(int half, int map, int base_half, int word, bool exchange)
    {
        if (exchange) std::swap(h->T[0].phidden, h->T[1].phidden);
        if (int rc = run(MBOTS_TK_MOVE, [&] {
                return mbots::launch_materialize_hidden(h->S, h->lazy_rows + word, h->hid_map2[map],
                                                        h->T[base_half].phidden, h->T[half].phidden, st);
            }))
            return rc;
        // (a graph that recorded the gather repeats it over 0 rows: the state it
        // ends is the host's, not the device's at a replay)
        HIP_TRY(mbots::launch_raise_flag(h->lazy_rows + word, 0u, st));
        return MBOTS_OK;
    }
    int gather_prev_action(int half, int par, bool base_prev)
    {
        const mbots::ObsTable &b = h->T[half ^ 1];
        if (int rc = run(MBOTS_TK_MOVE, [&] {
                return mbots::launch_materialize_action(h->S, h->lazy_rows + 2 + par, h->src_of2[par],
                                                        base_prev ? b.paction : b.action, h->T[half].paction, st);
            }))
            return rc;
        HIP_TRY(mbots::launch_raise_flag(h->lazy_rows + 2 + par, 0u, st));   // (as gather_hidden)
        return MBOTS_OK;
    }
    int copy_out(bool action, bool hidden)
    {
        HIP_TRY(hipSetDevice(h->device));
        if (int rc = sync_totals(h)) return rc;
        const size_t N = h->h_totals[mbots::kTotRows];   // the shard ghost's rows included
        const mbots::ObsTable &t = h->T[h->defer.tb];
        return timed(h, MBOTS_TK_MOVE, st, [&] {
            hipError_t e = hipSuccess;
            if (action && N)
                e = hipMemcpyAsync(t.action, t.paction, N * 6 * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && hidden && N)
                e = hipMemcpyAsync(t.hidden, t.phidden, N * mbots::kHidden * sizeof(float), hipMemcpyDeviceToDevice, st);
            return e;
        });
    }
    int wait_prev_sensor()
    {
        HIP_TRY(hipSetDevice(h->device));
        return h->sched.wait_prev_sensor(*this);
    }
};
// `st` is being captured into a graph (an entry point that refuses it)
bool capturing(mbots_handle *h, hipStream_t st) { return Exec{h, st}.capturing(); }
// the poisoning check of an entry point that takes no stream: it runs on the
// stream of the manager's last call
int capture_guard(mbots_handle *h)
{
    Exec ex{h, last_stream(h)};
    return h->sched.guard(ex, mbots::sched::kCaller);
}
mbots::defer::Env defer_env(const mbots_handle *h, bool capturing)
{
    return {capturing, h->sched.graph_exists(), h->pa_on, h->sched.mode.k1_finder && MB_FINDER_PSEM_BY_SENSOR};
}
static_assert(mbots::defer::kPartAH == mbots::kMoveAH && mbots::defer::kPartSensor == mbots::kMoveSensor &&
                  mbots::defer::kPartPrevAH == mbots::kMovePrevAH && mbots::defer::kPartPrev6 == mbots::kMovePrev6,
              "mbots_defer.hpp names launch_move's parts");
// the stream the manager last launched on is being captured into a graph
bool capturing_now(mbots_handle *h) { return capturing(h, last_stream(h)); }

int sync_totals(mbots_handle *h)
{
    // the step's row counts are final once synchronised: later accessors of the
    // same step skip the runtime calls (the reference loop reads ~10 views per
    // step and is host-bound at small world counts, scripts/refhost.py) -- not
    // once graphs exist, whose replays change the counts behind the host's back
    if (int rc = capture_guard(h)) return rc;
    if (h->totals_ok && !h->sched.graph_exists()) return MBOTS_OK;
    HIP_TRY(hipSetDevice(h->device));
    // a host-side row count during stream capture would be the capture-time
    // count baked into every replay (and the event wait is not capturable)
    if (capturing_now(h))
        return fail(MBOTS_E_INVALID,
                    "needs the host-side agent count, which is not available while the stream is "
                    "captured into a graph: capture only step / shift_observations / "
                    "write_synthetic_actions / join (device-side writers), read accessors after replay");
    HIP_TRY(hipEventSynchronize(h->ev[mbots::sched::kTotals]));
    h->totals_ok = true;
    return MBOTS_OK;
}

// episodes: every world's age is the manager's while no reset pass runs
int fill_ages(mbots_handle *h, hipStream_t st)
{
    if (capturing(h, st))
        return fail(MBOTS_E_INVALID, "the episode-step export of an unarmed manager cannot be captured into a graph");
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->age, (int)std::min<uint64_t>(h->age0, 0x7FFFFFFFu), h->S.W, st));
    return MBOTS_OK;
}
// arm the manager (on `st`, which the manager's calls are ordered on): from
// the next step on every step runs the reset pass
int arm(mbots_handle *h, hipStream_t st)
{
    if (h->armed) return MBOTS_OK;
    if (capturing(h, st))
        return fail(MBOTS_E_INVALID, "a manager cannot be armed for episodes while its stream is being captured: "
                                     "export MBOTS_EXPORT_RESET, call mbots_reset_worlds or set an episode length "
                                     "before the capture begins");
    if (int rc = fill_ages(h, st)) return rc;
    h->armed = true;
    return MBOTS_OK;
}

int record_totals(mbots_handle *h, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(h->h_totals, h->S.totals, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           st));
    HIP_TRY(hipEventRecord(h->ev[mbots::sched::kTotals], st));
    return MBOTS_OK;
}

// the trajectory window emptied (host bookkeeping only: its slots are a ring)
void traj_empty(mbots_handle *h)
{
    h->traj.n = h->traj.known = 0;
    h->traj.w.base = 0;
    h->traj.computed = false;
    h->traj.seq_valid = false;
}

// everything a window holds beside its main allocation (HIP mode: after the
// device has drained)
void traj_free_extras(mbots_handle *h)
{
    auto &tj = h->traj;
    if (h->cpu) {
        std::free(tj.idx);
    } else {
        if (tj.idx) (void)hipFree(tj.idx);
        if (tj.tabs) (void)hipFree((void *)tj.tabs);
        if (tj.h_tabs) (void)hipHostFree((void *)tj.h_tabs);
        if (tj.ev_tabs) (void)hipEventDestroy(tj.ev_tabs);
    }
    tj.idx = nullptr;
    tj.idx_cap = 0;
    tj.tabs = tj.h_tabs = nullptr;
    tj.ev_tabs = nullptr;
}

}  // namespace

// checkpoint segments (mbots_save_checkpoint / mbots_load_checkpoint)
namespace {
struct CkptHeader {
    char magic[8];
    uint32_t version, num_worlds, cap, A, world_offset, flags, seed, n_rows;
    uint64_t bytes;
    uint32_t sensed, pad;   // 4: whether a sensor had run (the finder slots are its)
};
// 3: totals[kTotRows] (every table row, the shard ghost's included) is part
// of the state and must equal the header's n_rows; 4: `sensed`;
// 5 (armed managers only; the others keep writing 4): the per-world episode,
// age and pending reset flags as three trailing segments, the episode length
// in `pad`
constexpr uint32_t kCkptVersion = 4;
constexpr uint32_t kCkptVersionEpisodes = 5;

struct Seg {
    void *p;
    size_t bytes;
};

// the first kSlotSegs segments are per-slot columns ([world][cap]); `cap`:
// the capacity the segments are sized for (0: the manager's)
constexpr size_t kSlotSegs = 11;
std::vector<Seg> ckpt_segments(mbots_handle *h, mbots::ObsTable &t, uint32_t n_rows, uint32_t cap = 0)
{
    using namespace mbots;
    SimState &S = h->S;
    const size_t W = S.W, rows = W * (cap ? cap : h->cfg.agent_capacity), N = n_rows;
    std::vector<Seg> v = {
        {S.x, rows * 4}, {S.y, rows * 4}, {S.rw, rows * 4}, {S.rz, rows * 4},
        {S.species, rows * 4}, {S.health, rows * 4}, {S.finder, rows * 4}, {S.obsrow, rows * 4},
        {S.sur0, rows * 4}, {S.sur1, rows * 4}, {S.stats, rows * 4},
        {S.n, W * 4}, {S.ctr, W * 4}, {S.key, W * 8}, {S.food, W * kNumChunks * 8},
        {S.food_rot, W * kNumPkg * 4},
        {S.cur_food, W * 4}, {S.sreward, W * kNumSpecies * 4}, {S.scount, W * kNumSpecies * 4},
        {S.row_base, W * kNumSpecies * 4}, {S.world_off, W * 4}, {S.overflow, W * 4},
        {S.totals, 8 * 4}, {S.agent_steps, 8},
        {t.species, N * 4}, {t.pos, N * 8}, {t.health, N * 4}, {t.sur, N * 8}, {t.reward, N * 4},
        {t.action, N * 24}, {t.stats, N * 16}, {t.hidden, N * kHidden * 4},
        {t.sem, N * kSensor}, {t.depth, N * kSensor},
        {t.pspecies, N * 4}, {t.ppos, N * 8}, {t.phealth, N * 4}, {t.psur, N * 8},
        {t.preward, N * 4}, {t.paction, N * 24}, {t.pstats, N * 16}, {t.phidden, N * kHidden * 4},
        {t.psem, N * kSensor}, {t.pdepth, N * kSensor},
    };
    return v;
}

// version 5's trailing segments
std::vector<Seg> ckpt_episode_segments(mbots_handle *h)
{
    const size_t W = h->S.W;
    return {{h->episode, W * 4}, {h->age, W * 4}, {h->reset_flags, W * 4}};
}

size_t ckpt_bytes(const std::vector<Seg> &v)
{
    size_t b = sizeof(CkptHeader);
    for (const Seg &s : v) b += s.bytes;
    return b;
}
// rollout records on the host (CPU mode, and the learner side of a gather
// that landed in host memory): the layout of include/mbots.h, the values of
// pack_rollout_kernel / unpack_rollout_kernel (plain bit copies and the
// uint8 / int8 -> f32 conversions of construct_obs)
void pack_rollout_host(const int8_t *sem, const uint8_t *depth, const int32_t *health, const float *pos,
                       const float *sur, const float *reward, const int32_t *stats, uint64_t n, uint8_t *out)
{
    const size_t rec = depth ? MBOTS_ROLLOUT_BYTES_DEPTH : MBOTS_ROLLOUT_BYTES;
    for (uint64_t r = 0; r < n; ++r) {
        uint8_t *o = out + r * rec;
        memcpy(o, sem + r * mbots::kSensor, 32);
        memcpy(o + 32, health + r, 4);
        memcpy(o + 36, pos + 2 * r, 8);
        memcpy(o + 44, sur + 2 * r, 8);
        memcpy(o + 52, reward + r, 4);
        for (int k = 0; k < 4; ++k) o[56 + k] = (uint8_t)stats[4 * r + k];
        memset(o + 60, 0, 4);
        if (depth) memcpy(o + 64, depth + r * mbots::kSensor, 32);
    }
}

void unpack_rollout_host(const uint8_t *recs, uint64_t n, bool with_depth, float *obs, float *reward,
                         int32_t *stats)
{
    const size_t rec = with_depth ? MBOTS_ROLLOUT_BYTES_DEPTH : MBOTS_ROLLOUT_BYTES;
    for (uint64_t r = 0; r < n; ++r) {
        const uint8_t *q = recs + r * rec;
        float *o = obs + r * 69;
        const uint8_t *d = with_depth ? q + 64 : q;
        for (int c = 0; c < 32; ++c) o[c] = (float)d[c];
        memcpy(o + 32, q + 32, 12);   // health bits, position
        for (int c = 0; c < 32; ++c) o[35 + c] = (float)(int8_t)q[c];
        memcpy(o + 67, q + 44, 8);    // surroundings
        if (reward) memcpy(reward + r, q + 52, 4);
        if (stats)
            for (int k = 0; k < 4; ++k) stats[4 * r + k] = q[56 + k];
    }
}

// learner records on the host (CPU mode, and a gather that landed in host
// memory): the layout of include/mbots.h, the values of pack_learner_kernel /
// unpack_learner_kernel
void pack_learner_host(const mbots::cpu::Table &t, bool fixd, uint64_t n, uint8_t *out)
{
    const size_t rec = fixd ? MBOTS_LEARNER_BYTES_DEPTH : MBOTS_LEARNER_BYTES;
    for (uint64_t r = 0; r < n; ++r) {
        uint8_t *o = out + r * rec;
        pack_rollout_host(t.sem.data() + r * mbots::kSensor, nullptr, t.health.data() + r, t.pos.data() + 2 * r,
                          t.sur.data() + 2 * r, t.reward.data() + r, t.stats.data() + 4 * r, 1, o);
        memcpy(o + 64, t.psem.data() + r * mbots::kSensor, 32);
        memcpy(o + 96, t.phealth.data() + r, 4);
        memcpy(o + 100, t.ppos.data() + 2 * r, 8);
        memcpy(o + 108, t.psur.data() + 2 * r, 8);
        memcpy(o + 116, t.action.data() + 6 * r, 24);
        memset(o + 140, 0, 4);
        memcpy(o + 144, t.hidden.data() + mbots::kHidden * r, 64);
        memcpy(o + 208, t.phidden.data() + mbots::kHidden * r, 64);
        if (fixd) {
            memcpy(o + 272, t.depth.data() + r * mbots::kSensor, 32);
            memcpy(o + 304, t.pdepth.data() + r * mbots::kSensor, 32);
        }
    }
}

// slim learner records on the host (CPU mode: every column materialised)
void pack_learner_slim_host(const mbots::cpu::Table &t, const int32_t *src_of, bool fixd, uint64_t n,
                            uint8_t *out)
{
    const size_t rec = fixd ? MBOTS_LEARNER_SLIM_BYTES_DEPTH : MBOTS_LEARNER_SLIM_BYTES;
    for (uint64_t r = 0; r < n; ++r) {
        uint8_t *o = out + r * rec;
        pack_rollout_host(t.sem.data() + r * mbots::kSensor, nullptr, t.health.data() + r, t.pos.data() + 2 * r,
                          t.sur.data() + 2 * r, t.reward.data() + r, t.stats.data() + 4 * r, 1, o);
        memcpy(o + 60, src_of + r, 4);
        memcpy(o + 64, t.psem.data() + r * mbots::kSensor, 32);
        memcpy(o + 96, t.phealth.data() + r, 4);
        memcpy(o + 100, t.ppos.data() + 2 * r, 8);
        memcpy(o + 108, t.psur.data() + 2 * r, 8);
        memset(o + 116, 0, 12);
        if (fixd) {
            memcpy(o + 128, t.depth.data() + r * mbots::kSensor, 32);
            memcpy(o + 160, t.pdepth.data() + r * mbots::kSensor, 32);
        }
    }
}

void unpack_learner_host(const uint8_t *recs, uint64_t n, bool fixd, const mbots_learner_out &o, bool slim = false,
                         int32_t *src = nullptr)
{
    const size_t rec = slim ? (fixd ? MBOTS_LEARNER_SLIM_BYTES_DEPTH : MBOTS_LEARNER_SLIM_BYTES)
                            : (fixd ? MBOTS_LEARNER_BYTES_DEPTH : MBOTS_LEARNER_BYTES);
    const size_t dc = slim ? 128 : 272, dp = slim ? 160 : 304;
    for (uint64_t r = 0; r < n; ++r) {
        const uint8_t *q = recs + r * rec;
        if (src) memcpy(src + r, q + 60, 4);
        for (int prev = 0; prev < 2; ++prev) {
            float *ob = prev ? o.prev_obs : o.obs;
            if (!ob) continue;
            ob += r * 69;
            const uint8_t *b = q + (prev ? 64 : 0);
            const uint8_t *d = fixd ? q + (prev ? dp : dc) : b;
            for (int c = 0; c < 32; ++c) ob[c] = (float)d[c];
            memcpy(ob + 32, b + 32, 12);   // health bits, position
            for (int c = 0; c < 32; ++c) ob[35 + c] = (float)(int8_t)b[c];
            memcpy(ob + 67, b + 44, 8);    // surroundings
        }
        if (o.reward) memcpy(o.reward + r, q + 52, 4);
        if (o.stats)
            for (int k = 0; k < 4; ++k) o.stats[4 * r + k] = q[56 + k];
        if (slim) continue;
        if (o.action) memcpy(o.action + 6 * r, q + 116, 24);
        if (o.hidden) memcpy(o.hidden + mbots::kHidden * r, q + 144, 64);
        if (o.prev_hidden) memcpy(o.prev_hidden + mbots::kHidden * r, q + 208, 64);
    }
}

}  // namespace

extern "C" {

const char *mbots_last_error(void) { return g_err.c_str(); }

int mbots_create(const mbots_config *cfg_in, mbots_handle **out)
{
    if (!cfg_in || !out) return fail(MBOTS_E_INVALID, "null argument");
    *out = nullptr;
    mbots_config cfg = *cfg_in;
    if (cfg.agent_capacity == 0) cfg.agent_capacity = 128;
    if (cfg.sensor_size == 0) cfg.sensor_size = 32;
    if (cfg.num_worlds == 0) return fail(MBOTS_E_INVALID, "num_worlds must be > 0");
    if (cfg.sensor_size != (uint32_t)mbots::kSensor)
        return fail(MBOTS_E_INVALID, "sensor_size must be 32 (mgr.hpp:19, entry.cpp:27)");
    static_assert(mbots::kMaxCap == (int)MBOTS_MAX_CAPACITY, "include/mbots.h");
    if (cfg.agent_capacity > (uint32_t)mbots::kMaxCap || cfg.agent_capacity < 4)
        return fail(MBOTS_E_INVALID, "agent_capacity must be in [4, " + std::to_string(mbots::kMaxCap) + "]");
    if (cfg.init_num_agents_per_world > cfg.agent_capacity)
        return fail(MBOTS_E_INVALID, "init_num_agents_per_world exceeds agent_capacity");
    if (cfg.init_num_agents_per_world < (uint32_t)mbots::kNumSpecies)
        return fail(MBOTS_E_INVALID, "init_num_agents_per_world must be >= 4");
    const uint64_t rows = (uint64_t)cfg.num_worlds * cfg.agent_capacity;
    if (rows >= (1ull << 31)) return fail(MBOTS_E_INVALID, "num_worlds * agent_capacity >= 2^31");
    if (cfg.exec_mode != MBOTS_EXEC_HIP && cfg.exec_mode != MBOTS_EXEC_CPU)
        return fail(MBOTS_E_INVALID, "exec_mode must be MBOTS_EXEC_HIP or MBOTS_EXEC_CPU");
    if (cfg.exec_mode == MBOTS_EXEC_CPU) {   // no HIP call on this path: runs without a GPU
        mbots_handle *h = new (std::nothrow) mbots_handle();
        if (!h) return fail(MBOTS_E_NOMEM, "host allocation failed");
        h->cfg = cfg;
        h->device = -1;
        try {
            h->cpu = std::make_unique<mbots::cpu::Sim>(cfg);
        } catch (const std::bad_alloc &) {
            delete h;
            return fail(MBOTS_E_NOMEM, "host allocation of the CPU-mode state failed");
        }
        *out = h;
        return MBOTS_OK;
    }

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg.gpu_id < 0 || cfg.gpu_id >= ndev)
        return fail(MBOTS_E_INVALID, "gpu_id out of range (" + std::to_string(ndev) + " devices)");
    HIP_TRY(hipSetDevice(cfg.gpu_id));

    mbots_handle *h = new mbots_handle();
    h->cfg = cfg;
    h->device = cfg.gpu_id;
    // the shard ghost is one more simulated world (the last), never exported
    h->S.W = cfg.num_worlds + ((cfg.flags & MBOTS_FLAG_SHARD_GHOST) ? 1u : 0u);
    h->S.Wx = cfg.num_worlds;
    Arena probe;
    const size_t bytes = layout(h, probe);
    if (hipMalloc(&h->arena.base, bytes) != hipSuccess) {
        delete h;
        return fail(MBOTS_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    h->arena.size = bytes;
    h->arena.used = 0;
    layout(h, h->arena);
    mbots::SimState &S = h->S;
    S.cap = cfg.agent_capacity;
    S.A = cfg.init_num_agents_per_world;
    S.world_offset = cfg.world_offset;
    S.flags = cfg.flags;
    S.seed = cfg.rand_seed;
    // the schedule the world count, the capacity and the environment ask for
    // (mbots_sched.hpp choose; settled below, once the signal words exist)
    h->sched.knobs = sched_knobs();
    h->sched.mode = mbots::sched::choose(S.W, S.cap, true, true, h->sched.knobs);
    S.k1_finder = h->sched.mode.k1_finder ? 1u : 0u;
    {
        // mixed capacity classes (round 6): above 128 slots the 128-slot K1
        // and sensor take every world that fits them and the class kernels
        // only the worlds K2 lists (DESIGN.md "Capacity"); MBOTS_MIXED=0 runs
        // every world in the class kernels
        S.mixed = (mixed_wanted() && S.cap > (uint32_t)mbots::kSmallCap && !h->sched.mode.k1_finder) ? 1u : 0u;
    }

    int rc = MBOTS_OK;
    auto check = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == MBOTS_OK)
            rc = fail(MBOTS_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    // (8 totals, then each scan tile's largest world: mbots_max_population)
    check(hipHostMalloc((void **)&h->h_totals, ((size_t)mbots::kTotMaxPop + S.ntiles) * sizeof(uint32_t),
                        hipHostMallocMapped),
          "hipHostMalloc");
    if (rc == MBOTS_OK)
        check(hipHostGetDevicePointer((void **)&S.totals_host, h->h_totals, 0),
              "hipHostGetDevicePointer");
    // (these ride on kernel dispatches as their stop events; synchronisation
    // only: no timestamps, and a device-scope release -- the host reads only the
    // pinned row counts, which K2 writes system-coherent and fences itself)
    constexpr unsigned kSyncEvent = hipEventDisableTiming | hipEventReleaseToDevice;
    check(hipEventCreateWithFlags(&h->ev[mbots::sched::kTotals], kSyncEvent), "hipEventCreateWithFlags");
    check(hipEventCreateWithFlags(&h->ev[mbots::sched::kHop], kSyncEvent), "hipEventCreateWithFlags");
    check(hipMalloc((void **)&h->reset_mark, (size_t)S.W * sizeof(int32_t)), "hipMalloc");
    if (rc == MBOTS_OK) check(hipMemset(h->reset_mark, 0, (size_t)S.W * sizeof(int32_t)), "hipMemset");
    {
        // the words hipStreamWaitValue32 polls (the runtime's wait kernel reads
        // them); without signal memory the waits stay event waits
        auto signal_word = [&](uint32_t *&p) {
            if (rc != MBOTS_OK) return;
            if (hipExtMallocWithFlags((void **)&p, 8, hipMallocSignalMemory) != hipSuccess) {
                (void)hipGetLastError();
                p = nullptr;
                return;
            }
            check(hipMemset(p, 0, 8), "hipMemset");
        };
        if (h->sched.mode.value_fork) signal_word(h->sig[mbots::sched::kFork]);
        if (h->sched.mode.value_join) signal_word(h->sig[mbots::sched::kJoin]);
        h->sched.mode = mbots::sched::choose(S.W, S.cap, h->sig[mbots::sched::kFork] != nullptr,
                                             h->sig[mbots::sched::kJoin] != nullptr, h->sched.knobs);
        S.sig_fork = h->sig[mbots::sched::kFork];
        // test hook: the epoch to count on from (near kEpochWrap, so a short
        // run crosses the wrap; include/mbots.h "Environment")
        if (const char *e = std::getenv("MBOTS_EPOCH_START"))
            h->sched.epoch = std::min<uint32_t>((uint32_t)std::strtoul(e, nullptr, 0), mbots::sched::kEpochWrap);
    }
    {
        // MBOTS_LAZY_PREV_ACTION=0: a lazy shift launches its Action gather, as
        // before the owed state (an A/B inside one build)
        const char *e = std::getenv("MBOTS_LAZY_PREV_ACTION");
        h->pa_on = !(e && e[0] == '0');
    }
    if (h->sched.mode.swap)
        check(hipEventCreateWithFlags(&h->ev[mbots::sched::kCallerEv], kSyncEvent), "hipEventCreateWithFlags");
    check(hipEventCreateWithFlags(&h->ev[mbots::sched::kJoin0], kSyncEvent), "hipEventCreateWithFlags");
    check(hipEventCreateWithFlags(&h->ev[mbots::sched::kJoin1], kSyncEvent), "hipEventCreateWithFlags");
    {
        // the sensor is the step's longer chain once the deferred Prev moves
        // left the caller's stream lighter: its stream gets the higher priority
        // (step -1.9 %, same box; DESIGN.md "Schedule")
        int least = 0, greatest = 0;
        check(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
        // (K1-finder mode: the caller's chain is the longer one, the sensor's the
        // filler)
        const int prio = h->sched.mode.aux_low() ? least : greatest;
        check(hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, prio),
              "hipStreamCreateWithPriority");
    }
    hipStream_t st = nullptr;
    check(hipMemsetAsync(h->arena.base, 0, bytes, st), "hipMemsetAsync");
    // Sim::Sim / initWorld (sim.cpp:1232-1256) + initial export of the rows
    check(mbots::upload_ray_table(S, st), "upload_ray_table");
    check(mbots::launch_init(S, st), "init_kernel");
    check(mbots::launch_tile_sum(S, 0, st), "tile_sum_kernel");
    check(mbots::launch_scan(S, 0, st), "scan_kernel");
    check(mbots::launch_export_rows(S, h->T[0], 1, st), "export_rows_kernel(init)");
    check(mbots::launch_move(S, h->T[1], h->T[0], 0, mbots::kMoveAll, st), "move_kernel(init)");
    if (rc == MBOTS_OK) rc = record_totals(h, st);
    check(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (rc != MBOTS_OK) {
        mbots_destroy(h);
        return rc;
    }
    // the init scan counted the initial population as agent-steps; reset
    unsigned long long zero = 0;
    check(hipMemcpy(S.agent_steps, &zero, sizeof(zero), hipMemcpyHostToDevice), "hipMemcpy");
    h->defer.tb = 0;
    h->defer.parity = 1;   // the init scan consumed buffer 0 and cleared buffer 1
    *out = h;
    return rc;
}

int mbots_destroy(mbots_handle *h)
{
    if (!h) return MBOTS_OK;
    if (h->cpu) {
        std::free(h->traj.mem);
        traj_free_extras(h);
        for (float *p : h->pol.mem) std::free(p);
        delete h;
        return MBOTS_OK;
    }
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (float *p : h->pol.mem) if (p) (void)hipFree(p);
    if (h->pol.table) (void)hipFree(h->pol.table);
    if (h->pol.draw) (void)hipFree(h->pol.draw);
    if (h->traj.mem) (void)hipFree(h->traj.mem);
    if (h->traj.h_count) (void)hipHostFree(h->traj.h_count);
    if (h->traj.h_S) (void)hipHostFree(h->traj.h_S);
    traj_free_extras(h);
    if (h->reset_mark) (void)hipFree(h->reset_mark);
    for (auto &p : h->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : h->pool) (void)hipEventDestroy(e);
    for (auto e : h->ev) if (e) (void)hipEventDestroy(e);
    for (auto p : h->sig) if (p) (void)hipFree(p);
    if (h->aux) (void)hipStreamDestroy(h->aux);
    if (h->h_totals) (void)hipHostFree(h->h_totals);
    if (h->flag_stage) (void)hipHostFree(h->flag_stage);
    if (h->flag_stage_dev) (void)hipFree(h->flag_stage_dev);
    if (h->ev_stage) (void)hipEventDestroy(h->ev_stage);
    if (h->render_list) (void)hipHostFree(h->render_list);
    if (h->render_list_dev) (void)hipFree(h->render_list_dev);
    if (h->ev_render_list) (void)hipEventDestroy(h->ev_render_list);
    if (h->arena.base) (void)hipFree(h->arena.base);
    for (char *p : h->retired) (void)hipFree(p);
    delete h;
    return MBOTS_OK;
}

// MBOTS_W_CAPACITY / MBOTS_E_CAPACITY once per rise of the dropped-agent total
// the smallest kernel capacity class holding `need` agents (the largest when
// none does)
static uint32_t capacity_class(uint64_t need)
{
    uint32_t c = (uint32_t)mbots::kSmallCap;
    while (c < MBOTS_MAX_CAPACITY && c < need) c *= 2;
    return c;
}

// mbots_set_auto_capacity: before a step that could overflow -- it adds at most
// n births (one per agent, sim.cpp:561-564) and A respawns (:830-834) to the
// largest world's n agents -- the smallest class that holds 2 n + A
static int auto_grow(mbots_handle *h)
{
    if (h->cfg.agent_capacity >= MBOTS_MAX_CAPACITY) return MBOTS_OK;   // (MBOTS_W_CAPACITY from here on)
    uint32_t n = 0;
    if (int rc = mbots_max_population(h, &n)) return rc;
    const uint64_t need = 2ull * n + h->cfg.init_num_agents_per_world;
    if (need <= h->cfg.agent_capacity) return MBOTS_OK;
    return mbots_grow_capacity(h, capacity_class(need));
}

static int capacity_report(mbots_handle *h, uint32_t dropped)
{
    if (dropped <= h->ovf_reported) return MBOTS_OK;
    const uint32_t was = h->ovf_reported;
    h->ovf_reported = dropped;
    g_err = std::to_string(dropped - was) + " births / respawns dropped at agent_capacity " +
            std::to_string(h->cfg.agent_capacity) + " (" + std::to_string(dropped) +
            " in total): the reference's worlds have no cap (sim.cpp:561-564, :830-834), so the run now "
            "differs from the reference's" +
            (h->cfg.agent_capacity < MBOTS_MAX_CAPACITY
                 ? "; raise agent_capacity (at most " + std::to_string(MBOTS_MAX_CAPACITY) + ")"
                 : " (" + std::to_string(MBOTS_MAX_CAPACITY) + " is the largest agent_capacity)");
    return (h->cfg.flags & MBOTS_FLAG_STRICT_CAPACITY) ? MBOTS_E_CAPACITY : MBOTS_W_CAPACITY;
}

int mbots_step(mbots_handle *h, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        if (h->auto_cap)
            if (int rc = auto_grow(h)) return rc;
        h->cpu->step();
        ++h->steps;
        return capacity_report(h, (uint32_t)std::min<uint64_t>(h->cpu->overflow(), 0xFFFFFFFFu));
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    int rc;
    Exec ex{h, st};
    unsigned long long cap_id = 0;
    if ((rc = ex.capture_of(mbots::sched::kCaller, cap_id))) return rc;
    const bool capturing = cap_id != 0;
    if (h->auto_cap) {
        // (the check reads the host-side population and a growth moves the
        // arena: neither can be part of a graph)
        if (capturing)
            return fail(MBOTS_E_INVALID, "automatic capacity cannot be captured into a graph: a step with "
                                         "mbots_set_auto_capacity enabled reads the largest population on the "
                                         "host and may move the manager's storage; disable it before capturing");
        if ((rc = auto_grow(h))) return rc;
    }
    // The launches in order -- reset pass, K1, (the halves) swap, K2, sensor,
    // K3a, prefetch move -- each after what the schedule (mbots_sched.hpp) makes
    // its queue wait for
    mbots::sched::Schedule &sched = h->sched;
    mbots::sched::Step sp;
    if ((rc = sched.begin_step(ex, sp))) return rc;
    const mbots::ObsTable &nxt = h->T[h->defer.tb ^ 1];
    const int par = h->defer.parity;
    // what the last step still owes the current half that this step reads, and
    // this step's part of the deferred columns (mbots_defer.hpp begin_step)
    const mbots::defer::Env env = defer_env(h, capturing);
    mbots::defer::StepPlan plan;
    if ((rc = h->defer.begin_step(ex, env, plan))) return rc;
    // K1 reads the learner's actions through the half's view (an aliased
    // Action column is its PrevAction), and so do this step's moves
    const mbots::ObsTable cur = src_view(h, h->defer.tb);
    if ((rc = sched.before_k1(ex, sp))) return rc;
    const hipStream_t kst = ex.queue(sp.kq);
    h->S.finder_from_state = h->sensed ? 0u : 1u;
    if (h->armed) {
        // the reset pass (episodes), before K1 on K1's stream
        if ((rc = sched.before_reset_pass(ex, sp))) return rc;
        const mbots::ResetArgs R{h->reset_flags, h->episode, h->age, h->ep_len, h->reset_mark};
        HIP_TRY(mbots::launch_reset_worlds(h->S, R, par, kst));
    } else {
        ++h->age0;
    }
    // K1 writes this step's old rows into the half the step before last used:
    // the sensor that read it (K1-finder mode: the sensor before the last one)
    // has been waited for above
    h->S.obsrow_out = h->obsrow_out2[par];
    if ((rc = timed(h, MBOTS_TK_WORLD_STEP, kst,
                    [&] { return mbots::launch_world_step(h->S, cur, par, kst); })))
        return rc;
    mbots::swap_state(h->S);
    // K2 writes the row counts into the pinned mirror; accessors and the
    // sensor's stream wait on ev[kTotals], carried by K2's own dispatch
    // (under stream capture -- a caller recording steps into a HIP graph -- the
    // fork / join events are recorded by hipEventRecord, the capturable form)
    if ((rc = sched.before_k2(ex, sp))) return rc;
    h->S.epoch = sp.k2_epoch;
    // this step's row bases and sensor order go to the buffer the step before
    // last used (its sensor has been waited for: above, or by the event join)
    h->S.row_base = h->row_base2[par];
    h->S.sorder = h->sorder2[par];
    // this step's row counts are K2's: no host read of them before it (ADVICE r4:
    // cleared here, after every materialisation above that may sync the last ones)
    h->totals_ok = false;
    // (owed PrevAction on: K2 also stores the table's rows where the gathers of
    // the owed columns read them -- the shift that follows launches nothing.
    // Not where a graph could replay the store over a count still in use)
    h->S.rows_out = plan.store_rows ? h->lazy_rows + par : nullptr;
    rc = timed(h, MBOTS_TK_SCAN, kst, [&] {
        return mbots::launch_scan(h->S, par, kst, h->ev[mbots::sched::kTotals], sp.plain_records);
    });
    h->S.rows_out = nullptr;
    h->maxpop_stale = false;
    h->S.epoch = 0;
    if (rc) return rc;
    // fork after K2: the sensor on its own stream
    if ((rc = sched.before_sensor(ex, sp))) return rc;
    // (K1-finder mode: the sensor also moves the last table's sensor rows into
    // its rows' prev-sensor columns, so no caller-stream wait is needed for them)
    if (env.psem_by_sensor) {
        h->S.psem_src = h->T[h->defer.tb].sem;
        h->S.pdepth_src = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) ? h->T[h->defer.tb].depth : nullptr;
    }
    h->S.list_par = (uint32_t)par;   // (mixed classes: this step's K2 lists)
    rc = timed(h, MBOTS_TK_SENSOR, h->aux, [&] {
        return mbots::launch_sensor(h->S, nxt, h->aux, h->ev[sp.join], sp.plain_records);
    });
    h->S.psem_src = nullptr;
    h->S.pdepth_src = nullptr;
    if (rc) return rc;
    h->sensed = true;
    if ((rc = sched.after_sensor(ex, sp))) return rc;
    // K3a's part of lazy HiddenState: the row map it composes or stores
    h->S.map_out = plan.map_out >= 0 ? h->hid_map2[plan.map_out] : nullptr;
    h->S.map_in = plan.map_in >= 0 ? h->hid_map2[plan.map_in] : nullptr;
    // this step's src_of goes to this parity's buffer (the last step's, which an
    // owed PrevAction may still read, stays); every reader from here on finds it
    // as S.src_of
    h->S.src_of = h->src_of2[par];
    if ((rc = timed(h, MBOTS_TK_EXPORT, st,
                    [&] { return mbots::launch_export_rows(h->S, nxt, 0, st); })))
        return rc;
    // (the prev sensor is the sensor's own part in K1-finder mode; moved here
    // instead, its source rows are the last sensor's, which this step's K1 did
    // not wait for in that mode)
    if ((plan.prefetch & mbots::kMoveSensor) && (rc = sched.wait_prev_sensor(ex))) return rc;
    if (plan.prefetch && (rc = timed(h, MBOTS_TK_MOVE, st, [&] {
                              return mbots::launch_move(h->S, cur, nxt, plan.lazy, plan.prefetch, st);
                          })))
        return rc;
    ++h->steps;
    h->defer.end_step(plan, env.psem_by_sensor);
    // capacity drops the device has published so far (K2's pinned mirror of a
    // recent step: no synchronisation)
    return capacity_report(h, __atomic_load_n(&h->h_totals[mbots::kTotOverflow], __ATOMIC_RELAXED));
}

int mbots_shift_observations(mbots_handle *h, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        h->cpu->shift_observations();
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    return h->defer.shift(ex, defer_env(h, ex.capturing()));
}

int mbots_num_agents(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->num_agents();
        return MBOTS_OK;
    }
    int rc = sync_totals(h);
    if (rc) return rc;
    *out = h->h_totals[0];
    return MBOTS_OK;
}

int mbots_export_on(mbots_handle *h, int32_t id, void *stream, mbots_tensor *out)
{
    using namespace mbots;
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        const int r = h->cpu->export_tensor(id, out);
        return r ? fail(r, "unknown export id " + std::to_string(id)) : MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    uint32_t N = 0;
    int rc = mbots_num_agents(h, &N);
    if (rc) return rc;
    // the view's deferred copies and joins go on the reader's stream, after
    // everything the manager enqueued (the step may have run on another)
    Exec ex{h, st};
    if ((rc = h->sched.enter(ex))) return rc;
    int want = 0;   // the deferred column the view names: real rows in its storage first
    switch (id) {
    case MBOTS_EXPORT_PREV_SPECIES: case MBOTS_EXPORT_PREV_POSITION: case MBOTS_EXPORT_PREV_HEALTH:
    case MBOTS_EXPORT_PREV_SURROUNDING: case MBOTS_EXPORT_PREV_REWARD: case MBOTS_EXPORT_PREV_STATS:
        want = defer::kPrev6; break;
    case MBOTS_EXPORT_PREV_ACTION: want = defer::kPrevAction; break;
    case MBOTS_EXPORT_PREV_HIDDEN_STATE: want = defer::kPrevHidden; break;
    case MBOTS_EXPORT_ACTION: want = defer::kAction; break;
    case MBOTS_EXPORT_HIDDEN_STATE: want = defer::kHidden; break;
    case MBOTS_EXPORT_PREV_SENSOR_SEMANTIC: case MBOTS_EXPORT_PREV_SENSOR_DEPTH: want = defer::kPrevSensor; break;
    default: break;
    }
    if (want && (rc = h->defer.require(ex, want, defer::How::Rows))) return rc;
    if (want == defer::kPrevSensor && h->sched.mode.k1_finder && (rc = h->sched.wait_sensor(ex))) return rc;   // the sensor moved them
    const ObsTable &t = h->T[h->defer.tb];
    const bool fixd = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    void *p = nullptr;
    int dt = MBOTS_DTYPE_INT32;
    int64_t rows = N, cols = 1;
    switch (id) {
    case MBOTS_EXPORT_RESET:   // the live flag array: whoever holds it may write it
        if ((rc = arm(h, st))) return rc;
        p = h->reset_flags; rows = h->cfg.num_worlds; break;
    case MBOTS_EXPORT_EPISODE: p = h->episode; rows = h->cfg.num_worlds; break;
    case MBOTS_EXPORT_EPISODE_STEP:
        // (unarmed: no pass keeps the ages; every world's is the manager's)
        if (!h->armed && (rc = fill_ages(h, st))) return rc;
        p = h->age; rows = h->cfg.num_worlds; break;
    case MBOTS_EXPORT_ACTION: p = t.action; cols = 6; break;
    case MBOTS_EXPORT_PREV_ACTION: p = t.paction; cols = 6; break;
    case MBOTS_EXPORT_HIDDEN_STATE: p = t.hidden; dt = MBOTS_DTYPE_FLOAT32; cols = kHidden; break;
    case MBOTS_EXPORT_PREV_HIDDEN_STATE: p = t.phidden; dt = MBOTS_DTYPE_FLOAT32; cols = kHidden; break;
    case MBOTS_EXPORT_REWARD: p = t.reward; dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_PREV_REWARD: p = t.preward; dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_DONE: p = h->done_zeros; break;
    case MBOTS_EXPORT_POSITION: p = t.pos; dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_PREV_POSITION: p = t.ppos; dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    // int32 health bits exported as a float32 view (types.hpp:119-124, mgr.cpp:329-346; B.2)
    case MBOTS_EXPORT_HEALTH: p = t.health; dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_PREV_HEALTH: p = t.phealth; dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_SURROUNDING: p = t.sur; dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_PREV_SURROUNDING: p = t.psur; dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_SENSOR_SEMANTIC:
        if ((rc = h->sched.wait_sensor(ex))) return rc;
        p = t.sem; dt = MBOTS_DTYPE_INT8; cols = kSensor; break;
    // SensorDepth exports the semantic buffer (sim.cpp:102-104, B.1) unless fixed
    case MBOTS_EXPORT_SENSOR_DEPTH:
        if ((rc = h->sched.wait_sensor(ex))) return rc;
        p = fixd ? (void *)t.depth : (void *)t.sem; dt = MBOTS_DTYPE_UINT8; cols = kSensor; break;
    case MBOTS_EXPORT_PREV_SENSOR_SEMANTIC: p = t.psem; dt = MBOTS_DTYPE_INT8; cols = kSensor; break;
    case MBOTS_EXPORT_PREV_SENSOR_DEPTH:
        p = fixd ? (void *)t.pdepth : (void *)t.psem; dt = MBOTS_DTYPE_UINT8; cols = kSensor; break;
    case MBOTS_EXPORT_STATS: p = t.stats; cols = 4; break;
    case MBOTS_EXPORT_PREV_STATS: p = t.pstats; cols = 4; break;
    case MBOTS_EXPORT_SENSOR_INDEX: {
        HIP_TRY(mbots::launch_sensor_index(h->S, h->sensor_index, st));
        HIP_TRY(hipStreamSynchronize(st));
        p = h->sensor_index;
        break;
    }
    case MBOTS_EXPORT_SPECIES_COUNT: p = h->S.scount; rows = h->cfg.num_worlds; cols = kNumSpecies; break;
    case MBOTS_EXPORT_SPECIES: p = t.species; break;
    case MBOTS_EXPORT_PREV_SPECIES: p = t.pspecies; break;
    default: return fail(MBOTS_E_INVALID, "unknown export id " + std::to_string(id));
    }
    out->data = p;
    out->dtype = dt;
    out->device = h->device;
    out->dims[0] = rows;
    out->dims[1] = cols;
    return MBOTS_OK;
}

int mbots_export(mbots_handle *h, int32_t id, mbots_tensor *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) return mbots_export_on(h, id, nullptr, out);
    // the reference's views are valid on any stream once the synchronous
    // step() returned (mgr.cpp:51-63): so are these, once this returns
    const int rc = mbots_export_on(h, id, last_stream(h), out);
    if (rc) return rc;
    if (!capturing_now(h)) HIP_TRY(hipStreamSynchronize(last_stream(h)));
    return MBOTS_OK;
}

int mbots_set_action(mbots_handle *h, uint32_t row, const int32_t action[6])
{
    if (!h || !action) return fail(MBOTS_E_INVALID, "null argument");
    uint32_t N = 0;
    int rc = mbots_num_agents(h, &N);
    if (rc) return rc;
    if (row >= N) return fail(MBOTS_E_RANGE, "agent row out of range");
    if (h->cpu) {
        memcpy(&h->cpu->table().action[(size_t)row * 6], action, 6 * sizeof(int32_t));
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = last_stream(h);
    Exec ex{h, st};
    if ((rc = h->defer.require(ex, mbots::defer::kAction, mbots::defer::How::Rows))) return rc;
    HIP_TRY(hipMemcpyAsync(h->T[h->defer.tb].action + (size_t)row * 6, action, 6 * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MBOTS_OK;
}

int mbots_agent_offset_for_world(mbots_handle *h, uint32_t world, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (world >= h->cfg.num_worlds) return fail(MBOTS_E_RANGE, "world out of range");
    if (h->cpu) {
        *out = h->cpu->world_offset_of(world);
        return MBOTS_OK;
    }
    int rc = sync_totals(h);
    if (rc) return rc;
    int32_t v = 0;
    HIP_TRY(hipMemcpy(&v, h->S.world_off + world, sizeof(v), hipMemcpyDeviceToHost));
    *out = (uint32_t)v;
    return MBOTS_OK;
}

int mbots_write_synthetic_actions(mbots_handle *h, uint32_t seed, uint32_t step,
                                  int32_t write_hidden, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        h->cpu->write_synthetic_actions(seed, step, write_hidden != 0);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    // the writer rewrites every live row's Action (and HiddenState with
    // write_hidden): an aliased column of those is simply written, not copied
    if ((rc = h->defer.require(ex, mbots::defer::kAction | (write_hidden ? mbots::defer::kHidden : 0),
                               mbots::defer::How::WriteAll)))
        return rc;
    return timed(h, MBOTS_TK_ACTIONS, st, [&] {
        return mbots::launch_synthetic_actions(h->S, h->T[h->defer.tb], seed, step, write_hidden, st);
    });
}

int mbots_construct_obs(mbots_handle *h, int32_t prev, float *out, uint64_t out_rows, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (out_rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "out_rows too large");
    if (h->cpu) {
        h->cpu->construct_obs(prev != 0, out, out_rows);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    // current semantic rows come from K3b (and in K1-finder mode the prev ones too)
    if ((!prev || h->sched.mode.k1_finder) && (rc = h->sched.wait_sensor(ex))) return rc;
    // The previous rows' health / position / surrounding: while the step's
    // deferred move of the six Prev* columns is still owed, gathered from the
    // other half along src_of inside this launch (what the move would write,
    // nothing materialised: the shift that follows in training_loop.py:135
    // makes the six the current columns, so the move is never run); the prev
    // sensor is moved (and remembered for the next step's prefetch)
    const mbots::defer::Deferred &d = h->defer;
    const bool gather6 = prev && d.six_owed();
    if (prev && (rc = h->defer.require(ex, mbots::defer::kPrevSensor, mbots::defer::How::Rows))) return rc;
    return timed(h, MBOTS_TK_OBS, st, [&] {
        return mbots::launch_construct_obs(h->S, h->T[d.tb], prev, d.prev_is_current() ? 1 : 0, out,
                                           (uint32_t)out_rows, st, gather6 ? &h->T[d.tb ^ 1] : nullptr,
                                           d.six_lazy() ? 1 : 0);
    });
}

int mbots_rollout_record_bytes(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    *out = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) ? MBOTS_ROLLOUT_BYTES_DEPTH : MBOTS_ROLLOUT_BYTES;
    return MBOTS_OK;
}

int mbots_pack_rollout(mbots_handle *h, void *out, uint64_t out_rows, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (out_rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "out_rows too large");
    const bool fixd = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    if (h->cpu) {
        const mbots::cpu::Table &t = h->cpu->table();
        const uint64_t n = std::min<uint64_t>(h->cpu->num_agents(), out_rows);
        pack_rollout_host(t.sem.data(), fixd ? t.depth.data() : nullptr, t.health.data(), t.pos.data(),
                          t.sur.data(), t.reward.data(), t.stats.data(), n, static_cast<uint8_t *>(out));
        return MBOTS_OK;
    }
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0) return fail(MBOTS_E_INVALID, "out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    if ((rc = h->sched.wait_sensor(ex))) return rc;   // the semantic / depth rows come from K3b
    return timed(h, MBOTS_TK_OBS, st, [&] {
        return mbots::launch_pack_rollout(h->S, h->T[h->defer.tb], out, (uint32_t)out_rows, st);
    });
}

int mbots_learner_record_bytes(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    *out = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) ? MBOTS_LEARNER_BYTES_DEPTH : MBOTS_LEARNER_BYTES;
    return MBOTS_OK;
}

int mbots_pack_learner(mbots_handle *h, void *out, uint64_t out_rows, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (out_rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "out_rows too large");
    const bool fixd = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    if (h->cpu) {
        pack_learner_host(h->cpu->table(), fixd, std::min<uint64_t>(h->cpu->num_agents(), out_rows),
                          static_cast<uint8_t *>(out));
        return MBOTS_OK;
    }
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0) return fail(MBOTS_E_INVALID, "out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    // every column the record carries in its storage: the step's deferred
    // moves the learner's reads need (and remembered, like the accessors', so
    // the next step prefetches them beside its sensor)
    if ((rc = h->defer.require_all(ex, true))) return rc;
    if ((rc = h->sched.wait_sensor(ex))) return rc;   // the sensor rows (and what it moved)
    return timed(h, MBOTS_TK_OBS, st, [&] {
        return mbots::launch_pack_learner(h->S, h->T[h->defer.tb], h->defer.prev_is_current() ? 1 : 0, out,
                                          (uint32_t)out_rows, st);
    });
}

int mbots_pack_learner_slim(mbots_handle *h, void *out, uint64_t out_rows, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (out_rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "out_rows too large");
    const bool fixd = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    if (h->cpu) {
        pack_learner_slim_host(h->cpu->table(), h->cpu->src_of(), fixd,
                               std::min<uint64_t>(h->cpu->num_agents(), out_rows), static_cast<uint8_t *>(out));
        return MBOTS_OK;
    }
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0) return fail(MBOTS_E_INVALID, "out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    // the sensor rows (and in K1-finder mode the prev sensor rows it moved);
    // in the joined schedule the last sensor's rows, the source of a prev
    // sensor still owed, were waited for by this step's K1
    if ((rc = h->sched.wait_sensor(ex))) return rc;
    const int tb = h->defer.tb;
    const mbots::ObsTable &last = h->T[tb ^ 1];
    return timed(h, MBOTS_TK_OBS, st, [&] {
        const mbots::defer::Deferred &d = h->defer;
        return mbots::launch_pack_learner_slim(h->S, h->T[tb], d.prev_is_current() ? 1 : 0,
                                               d.six_owed() ? &last : nullptr, d.six_lazy() ? 1 : 0,
                                               d.psem_owed() ? &last : nullptr, out, (uint32_t)out_rows, st);
    });
}

int mbots_unpack_learner_slim(const void *records, uint64_t rows, int32_t with_depth, int32_t device,
                              const mbots_learner_out *out, int32_t *src, void *stream)
{
    if (!out || (!records && rows)) return fail(MBOTS_E_INVALID, "null argument");
    if (out->action || out->hidden || out->prev_hidden)
        return fail(MBOTS_E_INVALID, "slim records carry no Action / HiddenState / PrevHiddenState");
    if (rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "rows too large");
    if (device < 0) {
        unpack_learner_host(static_cast<const uint8_t *>(records), rows, with_depth != 0, *out, true, src);
        return MBOTS_OK;
    }
    if ((reinterpret_cast<uintptr_t>(records) & 15u) != 0)
        return fail(MBOTS_E_INVALID, "records must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_unpack_learner_slim(records, (uint32_t)rows, with_depth ? 1 : 0, *out, src,
                                              as_stream(stream)));
    return MBOTS_OK;
}

int mbots_rebuild_learner(const int32_t *src, uint64_t rows, const int64_t *cur_counts, const int64_t *last_counts,
                          uint32_t ranks, const int32_t *last_action, const float *last_memory,
                          const float *last_hidden, uint64_t last_rows, int32_t *action, float *hidden,
                          float *prev_hidden, int32_t device, void *stream)
{
    if (!cur_counts || !last_counts || (rows && (!src || !action || !hidden || !prev_hidden)) ||
        (last_rows && (!last_action || !last_memory || !last_hidden)))
        return fail(MBOTS_E_INVALID, "null argument");
    if (ranks == 0 || ranks > MBOTS_MAX_LEARNER_RANKS)
        return fail(MBOTS_E_INVALID, "ranks must be in [1, " + std::to_string(MBOTS_MAX_LEARNER_RANKS) + "]");
    uint64_t cur = 0, last = 0;
    for (uint32_t i = 0; i < 4 * ranks; ++i) {
        if (cur_counts[i] < 0 || last_counts[i] < 0) return fail(MBOTS_E_INVALID, "negative row count");
        cur += (uint64_t)cur_counts[i];
        last += (uint64_t)last_counts[i];
    }
    if (cur != rows) return fail(MBOTS_E_INVALID, "cur_counts do not sum to rows");
    if (last != last_rows) return fail(MBOTS_E_INVALID, "last_counts do not sum to last_rows");
    if (rows > 0x7FFFFFFFull || last_rows > 0x7FFFFFFFull) return fail(MBOTS_E_INVALID, "rows too large");
    const mbots::RebuildPlan p = mbots::rebuild_plan(cur_counts, last_counts, ranks);
    if (device < 0) {
        // (a provenance outside the owning rank's last rows is refused, not read)
        for (uint64_t r = 0; r < rows; ++r) {
            const int32_t g = mbots::rebuild_row(p, (int32_t)r, src[r]);
            if (g >= (int64_t)last_rows) return fail(MBOTS_E_RANGE, "provenance outside the last table");
            for (int k = 0; k < 6; ++k) action[r * 6 + k] = g >= 0 ? last_action[(size_t)g * 6 + k] : 0;
            for (int k = 0; k < mbots::kHidden; ++k) {
                hidden[r * mbots::kHidden + k] = g >= 0 ? last_memory[(size_t)g * mbots::kHidden + k] : 0.0f;
                prev_hidden[r * mbots::kHidden + k] = g >= 0 ? last_hidden[(size_t)g * mbots::kHidden + k] : 0.0f;
            }
        }
        return MBOTS_OK;
    }
    for (const void *q : {(const void *)src, (const void *)last_action, (const void *)last_memory,
                          (const void *)last_hidden, (const void *)action, (const void *)hidden,
                          (const void *)prev_hidden})
        if (reinterpret_cast<uintptr_t>(q) & 7u) return fail(MBOTS_E_INVALID, "arrays must be 8-byte aligned");
    for (const void *q : {(const void *)last_memory, (const void *)last_hidden, (const void *)hidden,
                          (const void *)prev_hidden})
        if (reinterpret_cast<uintptr_t>(q) & 15u) return fail(MBOTS_E_INVALID, "float arrays must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_rebuild_learner(p, src, (uint32_t)rows, (uint32_t)last_rows, last_action, last_memory,
                                          last_hidden, action, hidden, prev_hidden, as_stream(stream)));
    return MBOTS_OK;
}

int mbots_unpack_learner(const void *records, uint64_t rows, int32_t with_depth, int32_t device,
                         const mbots_learner_out *out, void *stream)
{
    if (!out || (!records && rows)) return fail(MBOTS_E_INVALID, "null argument");
    if (rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "rows too large");
    if (device < 0) {
        unpack_learner_host(static_cast<const uint8_t *>(records), rows, with_depth != 0, *out);
        return MBOTS_OK;
    }
    if ((reinterpret_cast<uintptr_t>(records) & 15u) != 0)
        return fail(MBOTS_E_INVALID, "records must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_unpack_learner(records, (uint32_t)rows, with_depth ? 1 : 0, *out, as_stream(stream)));
    return MBOTS_OK;
}

int mbots_max_population(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->max_population();
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (!h->S.track_maxpop) {   // the first call: K2 publishes the tile maxima from the next step on
        h->S.track_maxpop = 1u;
        h->maxpop_stale = true;
    }
    if (h->maxpop_stale) {   // (after a checkpoint load or before tracking, until the next step's K2)
        HIP_TRY(hipDeviceSynchronize());
        std::vector<int32_t> n(h->S.W);
        HIP_TRY(hipMemcpy(n.data(), h->S.n, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        int32_t mx = 0;
        for (int32_t v : n) mx = std::max(mx, v);
        *out = (uint32_t)mx;
        return MBOTS_OK;
    }
    // the last step's K2 published each tile's largest world with the row
    // counts: waiting for it waits for K2 only, not for the step's sensor or
    // the caller's chain
    if (int rc = sync_totals(h)) return rc;
    uint32_t mx = 0;
    for (uint32_t t = 0; t < h->S.ntiles; ++t)
        mx = std::max(mx, __atomic_load_n(&h->h_totals[mbots::kTotMaxPop + t], __ATOMIC_RELAXED));
    *out = mx;
    return MBOTS_OK;
}

int mbots_num_rows(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->num_rows();
        return MBOTS_OK;
    }
    int rc = sync_totals(h);
    if (rc) return rc;
    *out = h->h_totals[mbots::kTotRows];
    return MBOTS_OK;
}

int mbots_write_actions(mbots_handle *h, const int32_t *action, const float *hidden, uint64_t rows, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    uint32_t N = 0, R = 0;
    int rc = mbots_num_agents(h, &N);
    if (!rc) rc = mbots_num_rows(h, &R);
    if (rc) return rc;
    if (rows != N && rows != R) return fail(MBOTS_E_INVALID, "rows must be num_agents() or num_rows()");
    if (h->cpu) {
        mbots::cpu::Table &t = h->cpu->table();
        if (action && rows) memcpy(t.action.data(), action, rows * 6 * sizeof(int32_t));
        if (hidden && rows) memcpy(t.hidden.data(), hidden, rows * mbots::kHidden * sizeof(float));
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    if ((rc = h->sched.enter(ex))) return rc;
    const int tb = h->defer.tb;
    // a column written only in part keeps its other rows: copied out of an
    // aliased Prev storage first; a column written whole is simply written
    if ((rc = h->defer.require(ex, (action ? mbots::defer::kAction : 0) | (hidden ? mbots::defer::kHidden : 0),
                               rows < R ? mbots::defer::How::WritePart : mbots::defer::How::WriteAll)))
        return rc;
    const mbots::ObsTable &t = h->T[tb];
    if (action && rows) HIP_TRY(hipMemcpyAsync(t.action, action, rows * 6 * sizeof(int32_t), hipMemcpyDefault, st));
    if (hidden && rows)
        HIP_TRY(hipMemcpyAsync(t.hidden, hidden, rows * mbots::kHidden * sizeof(float), hipMemcpyDefault, st));
    return MBOTS_OK;
}

int mbots_unpack_rollout(const void *records, uint64_t rows, int32_t with_depth, int32_t device, float *obs,
                         float *reward, int32_t *stats, void *stream)
{
    if ((!records || !obs) && rows) return fail(MBOTS_E_INVALID, "null argument");
    if (rows > 0xFFFFFFFFull) return fail(MBOTS_E_INVALID, "rows too large");
    if (device < 0) {
        unpack_rollout_host(static_cast<const uint8_t *>(records), rows, with_depth != 0, obs, reward, stats);
        return MBOTS_OK;
    }
    if ((stats && (reinterpret_cast<uintptr_t>(stats) & 15u)) || (reinterpret_cast<uintptr_t>(records) & 15u))
        return fail(MBOTS_E_INVALID, "records and stats must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_unpack_rollout(records, (uint32_t)rows, with_depth ? 1 : 0, obs, reward, stats,
                                         as_stream(stream)));
    return MBOTS_OK;
}

int mbots_join(mbots_handle *h, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) return MBOTS_OK;   // synchronous: nothing outstanding
    HIP_TRY(hipSetDevice(h->device));
    Exec ex{h, as_stream(stream)};
    return h->sched.join(ex);
}

int mbots_record_sensor_done(mbots_handle *h, void *event)
{
    if (!h || !event) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu || !h->sched.sensor_launched()) return fail(MBOTS_E_INVALID, "no sensor launched on the device");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(event), h->aux));
    return MBOTS_OK;
}

int mbots_agent_steps(mbots_handle *h, uint64_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->agent_steps();
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, h->S.agent_steps, sizeof(v), hipMemcpyDeviceToHost));
    *out = v;
    return MBOTS_OK;
}

int mbots_overflow(mbots_handle *h, uint64_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->overflow();
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> v(h->cfg.num_worlds);
    HIP_TRY(hipMemcpy(v.data(), h->S.overflow, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t s = 0;
    for (uint32_t x : v) s += x;
    *out = s;
    return MBOTS_OK;
}

// ---- checkpoint / restore (absent in the reference) ----
// Blob: header + the live state after the last step: agent SoA columns (all
// W x cap slots), per-world arrays, and the first N rows of every column of the
// current export table.  Restoring into a manager of the same configuration
// puts the table in half 0, clears the scan tiles and continues bit-exactly.
int mbots_checkpoint_size(mbots_handle *h, uint64_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        *out = h->cpu->checkpoint_bytes();
        return MBOTS_OK;
    }
    int rc = sync_totals(h);
    if (rc) return rc;
    *out = ckpt_bytes(ckpt_segments(h, h->T[h->defer.tb], h->h_totals[mbots::kTotRows])) +
           (h->armed ? ckpt_bytes(ckpt_episode_segments(h)) - sizeof(CkptHeader) : 0);
    return MBOTS_OK;
}

int mbots_save_checkpoint(mbots_handle *h, void *dst, uint64_t bytes)
{
    if (!h || !dst) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        std::string err;
        const int r = h->cpu->save(dst, bytes, err);
        return r ? fail(r, err) : MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = capture_guard(h)) return rc;
    Exec ex{h, last_stream(h)};
    if (int rc0 = h->defer.require_all(ex, false)) return rc0;
    HIP_TRY(hipDeviceSynchronize());   // the sensor's finder / semantic rows included
    int rc = sync_totals(h);
    if (rc) return rc;
    const uint32_t n_rows = h->h_totals[mbots::kTotRows];   // the shard ghost's rows included
    auto segs = ckpt_segments(h, h->T[h->defer.tb], n_rows);
    if (h->armed)
        for (const Seg &s : ckpt_episode_segments(h)) segs.push_back(s);
    const size_t need = ckpt_bytes(segs);
    if (bytes < need) return fail(MBOTS_E_INVALID, "checkpoint buffer too small");
    CkptHeader hd{};
    memcpy(hd.magic, "MBOTSCK", 8);
    hd.version = h->armed ? kCkptVersionEpisodes : kCkptVersion;
    hd.pad = h->armed ? h->ep_len : 0u;
    hd.num_worlds = h->cfg.num_worlds;
    hd.cap = h->cfg.agent_capacity;
    hd.A = h->cfg.init_num_agents_per_world;
    hd.world_offset = h->cfg.world_offset;
    hd.flags = h->cfg.flags;
    hd.seed = h->cfg.rand_seed;
    hd.n_rows = n_rows;
    hd.bytes = need;
    hd.sensed = h->sensed ? 1u : 0u;
    char *p = static_cast<char *>(dst);
    memcpy(p, &hd, sizeof(hd));
    p += sizeof(hd);
    for (const Seg &s : segs) {
        if (s.bytes) HIP_TRY(hipMemcpy(p, s.p, s.bytes, hipMemcpyDeviceToHost));
        p += s.bytes;
    }
    return MBOTS_OK;
}

// the state a restore ends with (mbots_load_checkpoint, mbots_grow_capacity):
// the restored table is half 0, the scan tiles are clear, nothing is deferred,
// no sensor is outstanding and the device is idle
static int restored_reset(mbots_handle *h, bool sensed)
{
    HIP_TRY(hipMemset(h->S.tiles, 0, (size_t)2 * h->S.ntiles * mbots::kTileBuckets * 5 * sizeof(int32_t)));
    if (h->S.mixed) {
        // the first K1 after the load (parity 0) reads the class list of slot 1
        HIP_TRY(hipMemset(h->S.big_cnt, 0, 4 * sizeof(uint32_t)));
        HIP_TRY(mbots::launch_build_lists(h->S, 1, nullptr));
    }
    h->sched.idle_reset();   // (the device is idle; the next call is the first on its stream)
    h->defer.reset();   // (half 0, parity 0, nothing deferred)
    h->steps = 1;
    h->sensed = sensed;
    hipStream_t st = nullptr;
    h->totals_ok = false;
    int rc = record_totals(h, st);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    h->ovf_reported = h->h_totals[mbots::kTotOverflow];   // drops before the checkpoint were reported then
    h->maxpop_stale = true;
    return MBOTS_OK;
}

int mbots_load_checkpoint(mbots_handle *h, const void *src, uint64_t bytes)
{
    if (!h || !src) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        std::string err;
        const int r = h->cpu->load(src, bytes, err);
        if (r) return fail(r, err);
        h->ovf_reported = (uint32_t)std::min<uint64_t>(h->cpu->overflow(), 0xFFFFFFFFu);
        traj_empty(h);
        return MBOTS_OK;
    }
    if (bytes < sizeof(CkptHeader)) return fail(MBOTS_E_INVALID, "checkpoint truncated");
    CkptHeader hd;
    memcpy(&hd, src, sizeof(hd));
    if (memcmp(hd.magic, "MBOTSCK", 8) != 0 || (hd.version != kCkptVersion && hd.version != kCkptVersionEpisodes))
        return fail(MBOTS_E_INVALID, "not a checkpoint of this version");
    const bool episodes = hd.version == kCkptVersionEpisodes;
    // (another agent_capacity is fine when every world of the blob fits this
    // manager's: its per-slot columns are re-laid out, world by world -- a
    // learner growing its worlds' capacity, SimManager(agent_capacity="auto"))
    if (hd.num_worlds != h->cfg.num_worlds || hd.cap < 4 || hd.cap > (uint32_t)mbots::kMaxCap ||
        hd.A != h->cfg.init_num_agents_per_world || hd.world_offset != h->cfg.world_offset ||
        hd.flags != h->cfg.flags || hd.seed != h->cfg.rand_seed)
        return fail(MBOTS_E_INVALID, "checkpoint configuration differs from the manager's");
    const uint32_t cap = h->cfg.agent_capacity, cap_src = hd.cap;
    if (hd.n_rows > (uint64_t)h->S.W * cap)
        return fail(MBOTS_E_INVALID, "checkpoint row count out of range");
    if (int rc = capture_guard(h)) return rc;
    auto segs = ckpt_segments(h, h->T[0], hd.n_rows);
    auto segs_src = ckpt_segments(h, h->T[0], hd.n_rows, cap_src);
    if (episodes)
        for (const Seg &s : ckpt_episode_segments(h)) {
            segs.push_back(s);
            segs_src.push_back(s);
        }
    if (bytes < ckpt_bytes(segs_src) || hd.bytes != ckpt_bytes(segs_src))
        return fail(MBOTS_E_INVALID, "checkpoint size mismatch");
    {
        // the blob's own totals must agree with its header before anything is
        // overwritten (a mismatch used to leave the manager half
        // restored), and every world's population must fit this capacity
        const char *q = static_cast<const char *>(src) + sizeof(hd);
        for (const Seg &s : segs_src) {
            if (s.p == h->S.totals) {
                uint32_t tot[8];
                memcpy(tot, q, sizeof(tot));
                if (tot[mbots::kTotRows] != hd.n_rows || tot[0] > hd.n_rows)
                    return fail(MBOTS_E_INVALID, "checkpoint row count disagrees with its saved totals");
            }
            if (s.p == h->S.n) {
                for (size_t w = 0; w < h->S.W; ++w) {
                    int32_t n;
                    memcpy(&n, q + 4 * w, 4);
                    if (n < 0 || (uint32_t)n > cap)
                        return fail(MBOTS_E_INVALID, "a world of the checkpoint holds " + std::to_string(n) +
                                                         " agents, more than agent_capacity " + std::to_string(cap));
                }
            }
            q += s.bytes;
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    traj_empty(h);   // (the rows' provenance is stale after a load: the window does not inherit it)
    const char *p = static_cast<const char *>(src) + sizeof(hd);
    for (size_t i = 0; i < segs.size(); ++i) {
        const Seg &s = segs[i];
        if (i < kSlotSegs && cap != cap_src) {   // [world][cap_src] -> [world][cap]
            HIP_TRY(hipMemcpy2D(s.p, (size_t)cap * 4, p, (size_t)cap_src * 4, (size_t)std::min(cap, cap_src) * 4,
                                h->S.W, hipMemcpyHostToDevice));
        } else if (s.bytes) {
            HIP_TRY(hipMemcpy(s.p, p, s.bytes, hipMemcpyHostToDevice));
        }
        p += segs_src[i].bytes;
    }
    // episodes: a version-5 blob brings its manager's armed state along; a
    // version-4 one knows no episodes -- an armed manager stays armed, keeps its
    // episode length and starts every world at episode 0, age 0, no flag pending
    if (episodes) {
        h->armed = true;
        h->ep_len = hd.pad;
    } else {
        for (const Seg &s : ckpt_episode_segments(h)) HIP_TRY(hipMemset(s.p, 0, s.bytes));
        h->age0 = 0;
    }
    return restored_reset(h, hd.sensed != 0);
}

// ---- capacity growth in place (absent in the reference, whose worlds have no
// cap: sim.cpp:561-564, :830-834) ----
int mbots_capacity(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    *out = h->cfg.agent_capacity;
    return MBOTS_OK;
}

namespace {
// everything layout() sets
struct LayoutPtrs {
    mbots::SimState S;
    mbots::ObsTable T[2];
    int32_t *row_base2[2], *sorder2[2], *obsrow_out2[2], *done_zeros, *reset_flags, *sensor_index;
    int32_t *episode, *age;
    int32_t *hid_map2[2], *src_of2[2];
    uint32_t *lazy_rows;
};
LayoutPtrs layout_ptrs(const mbots_handle *h)
{
    return {h->S, {h->T[0], h->T[1]}, {h->row_base2[0], h->row_base2[1]}, {h->sorder2[0], h->sorder2[1]},
            {h->obsrow_out2[0], h->obsrow_out2[1]}, h->done_zeros, h->reset_flags, h->sensor_index,
            h->episode, h->age, {h->hid_map2[0], h->hid_map2[1]}, {h->src_of2[0], h->src_of2[1]},
            h->lazy_rows};
}
void set_layout_ptrs(mbots_handle *h, const LayoutPtrs &p)
{
    h->S = p.S;
    for (int k = 0; k < 2; ++k) {
        h->T[k] = p.T[k];
        h->row_base2[k] = p.row_base2[k];
        h->sorder2[k] = p.sorder2[k];
        h->obsrow_out2[k] = p.obsrow_out2[k];
        h->hid_map2[k] = p.hid_map2[k];
        h->src_of2[k] = p.src_of2[k];
    }
    h->lazy_rows = p.lazy_rows;
    h->done_zeros = p.done_zeros;
    h->reset_flags = p.reset_flags;
    h->sensor_index = p.sensor_index;
    h->episode = p.episode;
    h->age = p.age;
}
}  // namespace

int mbots_grow_capacity(mbots_handle *h, uint32_t new_capacity)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    const uint32_t cap_old = h->cfg.agent_capacity;
    if (new_capacity > (uint32_t)mbots::kMaxCap)
        return fail(MBOTS_E_INVALID, "agent_capacity must be in [4, " + std::to_string(mbots::kMaxCap) + "]");
    if (new_capacity < cap_old)
        return fail(MBOTS_E_INVALID, "mbots_grow_capacity cannot shrink (" + std::to_string(cap_old) + " -> " +
                                         std::to_string(new_capacity) +
                                         " slots): load a checkpoint into a smaller manager instead");
    if (h->cpu) {
        if (new_capacity == cap_old) return MBOTS_OK;
        std::string err;
        const int r = h->cpu->grow(new_capacity, err);
        if (r) return fail(r, err);
        h->cfg.agent_capacity = new_capacity;
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (capturing_now(h))
        return fail(MBOTS_E_INVALID, "grow_capacity moves the manager's storage and cannot be captured into a graph");
    if (int rc = capture_guard(h)) return rc;
    if (new_capacity == cap_old) return MBOTS_OK;
    if (h->sched.graph_exists())
        return fail(MBOTS_E_INVALID, "captured graphs pin the capacity: a step of this manager was captured into a "
                                     "graph, whose replays write through the current storage's pointers; create "
                                     "a new manager (or load a checkpoint into one) to change agent_capacity");
    if ((uint64_t)h->S.W * new_capacity >= (1ull << 31))
        return fail(MBOTS_E_INVALID, "num_worlds * agent_capacity >= 2^31");
    Exec ex{h, last_stream(h)};
    int rc = h->defer.require_all(ex, false);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());   // the sensor's finder / semantic rows included
    if ((rc = sync_totals(h))) return rc;
    const uint32_t n_rows = h->h_totals[mbots::kTotRows];   // the shard ghost's rows included
    // the old storage: what a checkpoint would save, and the row provenance
    const std::vector<Seg> from = ckpt_segments(h, h->T[h->defer.tb], n_rows);
    const int32_t *src_of_old = h->S.src_of;
    const std::vector<Seg> ep_from = ckpt_episode_segments(h);
    const LayoutPtrs old = layout_ptrs(h);
    const Arena old_arena = h->arena;
    h->cfg.agent_capacity = new_capacity;   // (layout() sizes by it)
    Arena fresh;
    const size_t bytes = layout(h, fresh);
    auto undo = [&] {
        set_layout_ptrs(h, old);
        h->cfg.agent_capacity = cap_old;
        h->arena = old_arena;
    };
    h->retired.reserve(h->retired.size() + 1);   // (so retiring the old arena below cannot throw)
    if (hipMalloc(&fresh.base, bytes) != hipSuccess) {
        (void)hipGetLastError();
        undo();
        return fail(MBOTS_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for agent_capacity " +
                                       std::to_string(new_capacity) + " failed; the manager keeps running at " +
                                       std::to_string(cap_old));
    }
    fresh.size = bytes;
    fresh.used = 0;
    h->arena = fresh;
    layout(h, h->arena);
    h->S.cap = new_capacity;
    const std::vector<Seg> to = ckpt_segments(h, h->T[0], n_rows);
    const std::vector<Seg> ep_to = ckpt_episode_segments(h);
    hipStream_t st = nullptr;
    auto move = [&]() -> hipError_t {
        // the per-slot columns lead the arena (layout()'s first takes) and the
        // kernel writes every slot of them: everything behind them is cleared,
        // as mbots_create clears it
        char *rest = reinterpret_cast<char *>(h->S.n);
        for (size_t i = 0; i < kSlotSegs; ++i)
            if (static_cast<char *>(to[i].p) + to[i].bytes > rest) rest = h->arena.base;
        hipError_t e = hipMemsetAsync(rest, 0, (size_t)(h->arena.base + bytes - rest), st);
        if (e != hipSuccess) return e;
        mbots::GrowCols c{};
        static_assert(kSlotSegs == (size_t)mbots::kGrowCols, "ckpt_segments");
        for (size_t i = 0; i < kSlotSegs; ++i) {
            c.src[i] = from[i].p;
            c.dst[i] = to[i].p;
        }
        if ((e = mbots::launch_grow_slots(c, (uint32_t)h->S.W, cap_old, new_capacity, st)) != hipSuccess) return e;
        for (size_t i = kSlotSegs; i < to.size(); ++i)
            if (to[i].bytes &&
                (e = hipMemcpyAsync(to[i].p, from[i].p, to[i].bytes, hipMemcpyDeviceToDevice, st)) != hipSuccess)
                return e;
        // (a checkpoint does not carry it: slim learner records packed before the
        // next step keep their provenance)
        if (n_rows && (e = hipMemcpyAsync(h->S.src_of, src_of_old, (size_t)n_rows * sizeof(int32_t),
                                          hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return e;
        for (size_t i = 0; i < ep_to.size(); ++i)   // episodes, ages and pending flags carry on
            if ((e = hipMemcpyAsync(ep_to[i].p, ep_from[i].p, ep_to[i].bytes, hipMemcpyDeviceToDevice, st)) !=
                hipSuccess)
                return e;
        if ((e = mbots::upload_ray_table(h->S, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    if (const hipError_t e = move(); e != hipSuccess) {
        (void)hipDeviceSynchronize();
        (void)hipFree(fresh.base);
        undo();
        return fail(MBOTS_E_HIP, std::string("mbots_grow_capacity: ") + hipGetErrorString(e));
    }
    // what mbots_create derives from the capacity
    h->sched.mode = mbots::sched::choose(h->S.W, h->S.cap, h->sig[mbots::sched::kFork] != nullptr,
                                         h->sig[mbots::sched::kJoin] != nullptr, h->sched.knobs);
    h->S.k1_finder = h->sched.mode.k1_finder ? 1u : 0u;
    h->S.mixed = (mixed_wanted() && h->S.cap > (uint32_t)mbots::kSmallCap && !h->sched.mode.k1_finder) ? 1u : 0u;
    h->retired.push_back(old_arena.base);
    const uint32_t reported = h->ovf_reported;
    const bool sensed = h->sensed;
    rc = restored_reset(h, sensed);
    h->ovf_reported = reported;   // (drops not yet reported stay owed: nothing was restored)
    return rc;
}

int mbots_set_auto_capacity(mbots_handle *h, int32_t enable)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    h->auto_cap = enable != 0;
    if (h->auto_cap && !h->cpu && !h->S.track_maxpop) {
        // K2 publishes the tile maxima from the next step on (not from the
        // first check on, a step later)
        h->S.track_maxpop = 1u;
        h->maxpop_stale = true;
    }
    return MBOTS_OK;
}

int mbots_release_retired(mbots_handle *h)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        h->cpu->release_retired();
        return MBOTS_OK;
    }
    if (h->retired.empty()) return MBOTS_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (capturing_now(h)) return fail(MBOTS_E_INVALID, "release_retired cannot be captured into a graph");
    HIP_TRY(hipDeviceSynchronize());   // (a caller's kernel may still read a retired view)
    for (char *p : h->retired) (void)hipFree(p);
    h->retired.clear();
    return MBOTS_OK;
}

int mbots_world_state(mbots_handle *h, uint32_t world, float *xy_rwrz, int32_t *sp_hp_finder,
                      uint64_t *food, uint32_t *food_rot, int32_t *n_out)
{
    using namespace mbots;
    if (!h || !xy_rwrz || !sp_hp_finder || !food || !n_out) return fail(MBOTS_E_INVALID, "null argument");
    if (world >= h->cfg.num_worlds) return fail(MBOTS_E_INVALID, "world out of range");
    if (h->cpu) {
        h->cpu->world_state(world, xy_rwrz, sp_hp_finder, food, food_rot, n_out);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const SimState &S = h->S;
    const size_t cap = h->cfg.agent_capacity, base = (size_t)world * cap;
    std::vector<float> f(cap);
    std::vector<int32_t> v(cap);
    const float *fc[4] = {S.x, S.y, S.rw, S.rz};
    for (int c = 0; c < 4; ++c) {
        HIP_TRY(hipMemcpy(f.data(), fc[c] + base, cap * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cap; ++i) xy_rwrz[i * 4 + c] = f[i];
    }
    const int32_t *ic[3] = {S.species, S.health, S.finder};
    for (int c = 0; c < 3; ++c) {
        HIP_TRY(hipMemcpy(v.data(), ic[c] + base, cap * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cap; ++i) sp_hp_finder[i * 3 + c] = v[i];
    }
    HIP_TRY(hipMemcpy(food, S.food + (size_t)world * kNumChunks, kNumChunks * 8, hipMemcpyDeviceToHost));
    if (food_rot)
        HIP_TRY(hipMemcpy(food_rot, S.food_rot + (size_t)world * kNumPkg, kNumPkg * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_out, S.n + world, 4, hipMemcpyDeviceToHost));
    return MBOTS_OK;
}

namespace {
// mbots_set_world_state's argument checks (everything but the population):
// the states actionSystem's clamp, the rotation steps and addFoodToChunk can
// leave, so a written scene is one the simulator could have reached
const char *scene_invalid(const float *a, uint32_t n_agents, const int32_t *food, uint32_t n_food)
{
    for (uint32_t i = 0; i < n_agents; ++i) {
        const float x = a[4 * i], y = a[4 * i + 1], rw = a[4 * i + 2], rz = a[4 * i + 3];
        if (!std::isfinite(x) || !std::isfinite(y) || x < 0.0f || x > mbots::kLx - 1.0f || y < 0.0f ||
            y > mbots::kLy - 1.0f)
            return "an agent position is not finite or outside [0, 127] x [0, 95]";
        const double d = (double)rw * rw + (double)rz * rz - 1.0;
        if (!std::isfinite(rw) || !std::isfinite(rz) || d > 1e-3 || d < -1e-3)
            return "an agent rotation is not finite or not a unit quaternion (|w^2 + z^2 - 1| > 1e-3)";
    }
    if (n_food > (uint32_t)mbots::kFoodCap) return "more than 30 food packages";
    int per_chunk[mbots::kNumChunks] = {};
    for (uint32_t k = 0; k < n_food; ++k) {
        const int32_t c = food[4 * k], x = food[4 * k + 1], y = food[4 * k + 2], rot = food[4 * k + 3];
        if (c < 0 || c >= mbots::kNumChunks) return "a food package's chunk is out of range";
        const int32_t lx = x - (c % mbots::kChunksX) * mbots::kChunkW, ly = y - (c / mbots::kChunksX) * mbots::kChunkW;
        if (lx < 0 || lx >= mbots::kChunkW || ly < 0 || ly >= mbots::kChunkW)
            return "a food package lies outside its chunk";
        if (rot < 0 || rot >= (1 << 22)) return "a food package's rotation is not a 22-bit quarter-turn fraction";
        if (++per_chunk[c] > mbots::kMaxPkg) return "more than 5 food packages in one chunk";
    }
    return nullptr;
}

// the packed records ([48] of 5 x (x | y << 4), live mask << 40) and rotations
// ([5][48]) of a package list: each chunk's slots fill from 0 in list order
void pack_food(const int32_t *food, uint32_t n_food, uint64_t *rec, uint32_t *rot)
{
    using namespace mbots;
    memset(rec, 0, kNumChunks * sizeof(uint64_t));
    memset(rot, 0, kNumPkg * sizeof(uint32_t));
    int used[kNumChunks] = {};
    for (uint32_t k = 0; k < n_food; ++k) {
        const int c = food[4 * k], q = used[c]++;
        const uint64_t lx = (uint64_t)(food[4 * k + 1] - (c % kChunksX) * kChunkW);
        const uint64_t ly = (uint64_t)(food[4 * k + 2] - (c / kChunksX) * kChunkW);
        rec[c] |= ((lx | (ly << 4)) << (8 * q)) | (1ull << (40 + q));
        rot[q * kNumChunks + c] = (uint32_t)food[4 * k + 3];
    }
}
}  // namespace

int mbots_set_world_state(mbots_handle *h, uint32_t world, const float *xy_rwrz, uint32_t n_agents,
                          const int32_t *food, uint32_t n_food)
{
    using namespace mbots;
    if (!h || (!xy_rwrz && n_agents) || (!food && n_food)) return fail(MBOTS_E_INVALID, "null argument");
    if (world >= h->cfg.num_worlds) return fail(MBOTS_E_INVALID, "world out of range");
    if (const char *why = scene_invalid(xy_rwrz, n_agents, food, n_food)) return fail(MBOTS_E_INVALID, why);
    uint64_t rec[kNumChunks];
    uint32_t rot[kNumPkg];
    pack_food(food, n_food, rec, rot);
    static const char *kPop = "the agent count differs from the world's population";
    if (h->cpu) {
        if (n_agents != h->cpu->population(world)) return fail(MBOTS_E_INVALID, kPop);
        h->cpu->set_world_state(world, xy_rwrz, rec, rot, (int32_t)n_food);
        traj_empty(h);   // (as HIP mode's checkpoint round trip does)
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = capture_guard(h)) return rc;
    if (capturing_now(h))
        return fail(MBOTS_E_INVALID, "set_world_state is a host-side write and cannot be captured into a graph");
    // the checkpoint path: save, patch the blob's segments (found by pointer
    // identity, as mbots_load_checkpoint finds S.n and S.totals), load -- the
    // load resets the lazy / pending / alias bookkeeping
    uint64_t bytes = 0;
    if (int rc = mbots_checkpoint_size(h, &bytes)) return rc;
    std::vector<char> blob(bytes);
    if (int rc = mbots_save_checkpoint(h, blob.data(), bytes)) return rc;
    CkptHeader hd;
    memcpy(&hd, blob.data(), sizeof(hd));
    const SimState &S = h->S;
    const size_t cap = h->cfg.agent_capacity, base = (size_t)world * cap;
    const auto segs = ckpt_segments(h, h->T[h->defer.tb], hd.n_rows);
    char *q = blob.data() + sizeof(hd);
    for (const Seg &s : segs) {   // the population first: nothing is patched on a mismatch
        if (s.p == S.n) {
            int32_t n;
            memcpy(&n, q + 4 * (size_t)world, 4);
            if (n < 0 || (uint32_t)n != n_agents) return fail(MBOTS_E_INVALID, kPop);
        }
        q += s.bytes;
    }
    q = blob.data() + sizeof(hd);
    for (const Seg &s : segs) {
        const float *const col[4] = {S.x, S.y, S.rw, S.rz};
        for (int c = 0; c < 4; ++c)
            if (s.p == col[c])
                for (uint32_t i = 0; i < n_agents; ++i) memcpy(q + 4 * (base + i), &xy_rwrz[4 * i + c], 4);
        if (s.p == S.food) memcpy(q + (size_t)world * kNumChunks * 8, rec, sizeof(rec));
        if (s.p == S.food_rot) memcpy(q + (size_t)world * kNumPkg * 4, rot, sizeof(rot));
        if (s.p == S.cur_food) {
            const int32_t nf = (int32_t)n_food;
            memcpy(q + 4 * (size_t)world, &nf, 4);
        }
        q += s.bytes;
    }
    return mbots_load_checkpoint(h, blob.data(), bytes);
}

// ---- episodes and resets (the reference registers WorldReset and keeps
// curWorldEpisode, sim.cpp:64-75, :1236-1240; its resetSystem is a stub,
// :302-305) ----
int mbots_reset_worlds(mbots_handle *h, const uint32_t *global_worlds, uint32_t n, const uint32_t *episodes,
                       void *stream)
{
    if (!h || (!global_worlds && n)) return fail(MBOTS_E_INVALID, "null argument");
    if (episodes)
        for (uint32_t k = 0; k < n; ++k)
            if (episodes[k] >= 0x7FFFFFFEu)
                return fail(MBOTS_E_INVALID, "episode " + std::to_string(episodes[k]) + " is out of range (< 2^31 - 2)");
    if (n == 0) return MBOTS_OK;
    if (h->cpu) {
        h->cpu->reset_worlds(global_worlds, n, episodes);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    if (ex.capturing())
        return fail(MBOTS_E_INVALID, "mbots_reset_worlds uploads its list from the host and cannot be captured into "
                                     "a graph: write the flags of MBOTS_EXPORT_RESET on the captured stream or "
                                     "between replays instead");
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    if ((rc = arm(h, st))) return rc;
    if ((rc = h->defer.require_prev_action_storage(ex))) return rc;   // (an unusual call: the owed column made real)
    const uint32_t W = h->S.W;   // (the shard ghost is world W - 1: global index world_offset + num_worlds)
    if (!h->flag_stage) {
        HIP_TRY(hipHostMalloc((void **)&h->flag_stage, (size_t)W * sizeof(int32_t), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&h->flag_stage_dev, (size_t)W * sizeof(int32_t)));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming));
    } else {
        HIP_TRY(hipEventSynchronize(h->ev_stage));   // the last call's upload has left the staging buffer
    }
    memset(h->flag_stage, 0, (size_t)W * sizeof(int32_t));
    bool any = false;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gw = global_worlds[k];
        if (gw < h->cfg.world_offset || gw - h->cfg.world_offset >= W) continue;   // another rank's
        h->flag_stage[gw - h->cfg.world_offset] = episodes ? (int32_t)(episodes[k] + 2u) : 1;
        any = true;
    }
    if (!any) return MBOTS_OK;
    HIP_TRY(hipMemcpyAsync(h->flag_stage_dev, h->flag_stage, (size_t)W * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(h->ev_stage, st));
    HIP_TRY(mbots::launch_set_flags(h->reset_flags, h->flag_stage_dev, W, st));
    return MBOTS_OK;
}

int mbots_set_episode_length(mbots_handle *h, uint32_t steps)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        h->cpu->set_episode_length(steps);
        return MBOTS_OK;
    }
    if (steps == h->ep_len) return MBOTS_OK;
    if (h->sched.graph_exists())
        return fail(MBOTS_E_INVALID, "captured graphs pin the episode length: a step of this manager was captured "
                                     "into a graph, whose replays carry the length they recorded");
    if (steps != 0 && !h->armed) {
        HIP_TRY(hipSetDevice(h->device));
        if (int rc = capture_guard(h)) return rc;
        if (int rc = arm(h, last_stream(h))) return rc;
    }
    h->ep_len = steps;
    return MBOTS_OK;
}

// ---- rasteriser (include/mbots.h "Rasteriser"; DESIGN.md "Rasteriser") ----
int mbots_render_palette(uint8_t rgb[36])
{
    if (!rgb) return fail(MBOTS_E_INVALID, "null argument");
    for (uint32_t c = 0; c < (uint32_t)mbots::kRenderClasses; ++c) {
        const uint32_t p = mbots::render_palette(c);
        rgb[3 * c] = (uint8_t)p;
        rgb[3 * c + 1] = (uint8_t)(p >> 8);
        rgb[3 * c + 2] = (uint8_t)(p >> 16);
    }
    return MBOTS_OK;
}

int mbots_render_worlds(mbots_handle *h, const uint32_t *worlds, uint32_t k, uint32_t scale,
                        const mbots_render_out *out, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (!out->cls && !out->slot && !out->rgb) return fail(MBOTS_E_INVALID, "mbots_render_worlds: no output asked for");
    if (!mbots::render_scale_ok(scale))
        return fail(MBOTS_E_INVALID, "mbots_render_worlds: scale " + std::to_string(scale) + " is not 1, 2, 4 or 8");
    if (((uintptr_t)out->cls | (uintptr_t)out->slot | (uintptr_t)out->rgb) & 3u)
        return fail(MBOTS_E_INVALID, "mbots_render_worlds: the outputs must be 4-byte aligned");
    // (the shard ghost is world num_worlds: never rendered)
    for (uint32_t i = 0; worlds && i < k; ++i)
        if (worlds[i] >= h->cfg.num_worlds)
            return fail(MBOTS_E_RANGE, "mbots_render_worlds: world " + std::to_string(worlds[i]) + " of " +
                                           std::to_string(h->cfg.num_worlds));
    if (!worlds && k > h->cfg.num_worlds)
        return fail(MBOTS_E_RANGE, "mbots_render_worlds: " + std::to_string(k) + " worlds of " +
                                       std::to_string(h->cfg.num_worlds));
    if ((uint64_t)k * (mbots::kRenderH * scale) >= (1ull << 31))
        return fail(MBOTS_E_INVALID, "mbots_render_worlds: too many images for one call");
    if (k == 0) return MBOTS_OK;
    const mbots::RenderOut ro{out->cls, out->slot, out->rgb};
    if (h->cpu) {
        h->cpu->render(worlds, k, scale, ro);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    if (ex.capturing())
        return fail(MBOTS_E_INVALID, "mbots_render_worlds cannot be captured into a graph (its world list is "
                                     "uploaded from the host, and a replay would read the state halves the capture "
                                     "recorded): render between replays");
    if (int rc = h->sched.enter(ex)) return rc;
    // In stream order the call follows the last step's K1 and K2 (on the
    // swapped schedule the caller's stream joined them after K2) and runs
    // beside its sensor, which writes nothing the kernel reads.  The next
    // step's K1 and reset pass, which overwrite what it reads, start after
    // everything enqueued here (the same stream, or the caller event): no wait of its
    // own is needed (DESIGN.md "Rasteriser").
    const uint32_t *list = nullptr;
    if (worlds) {
        if (k > h->render_list_cap) {
            // (rare: the last render may still read the old list)
            HIP_TRY(hipDeviceSynchronize());
            if (h->render_list) (void)hipHostFree(h->render_list);
            if (h->render_list_dev) (void)hipFree(h->render_list_dev);
            h->render_list = h->render_list_dev = nullptr;
            h->render_list_cap = 0;
            const uint32_t cap = std::max<uint32_t>(k, 64u);
            HIP_TRY(hipHostMalloc((void **)&h->render_list, (size_t)cap * sizeof(uint32_t), hipHostMallocDefault));
            HIP_TRY(hipMalloc((void **)&h->render_list_dev, (size_t)cap * sizeof(uint32_t)));
            h->render_list_cap = cap;
            if (!h->ev_render_list) HIP_TRY(hipEventCreateWithFlags(&h->ev_render_list, hipEventDisableTiming));
        } else {
            HIP_TRY(hipEventSynchronize(h->ev_render_list));   // the last upload has left the pinned list
        }
        memcpy(h->render_list, worlds, (size_t)k * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(h->render_list_dev, h->render_list, (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice,
                               st));
        HIP_TRY(hipEventRecord(h->ev_render_list, st));
        list = h->render_list_dev;
    }
    HIP_TRY(mbots::launch_render(h->S, list, k, scale, ro, st));
    return MBOTS_OK;
}

int mbots_enable_kernel_timing(mbots_handle *h, int32_t enable)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) return MBOTS_OK;   // no kernels
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    for (auto &p : h->pending) { h->pool.push_back(p.a); h->pool.push_back(p.b); }
    h->pending.clear();
    for (int k = 0; k < MBOTS_TK_COUNT; ++k) { h->acc_ms[k] = 0.0; h->acc_n[k] = 0; }
    h->timing = enable != 0;
    return MBOTS_OK;
}

int mbots_schedule_info(mbots_handle *h, uint32_t out[4])
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        out[0] = h->cpu->armed() ? 32u : 0u;
        out[1] = out[2] = 0;
        out[3] = (uint32_t)h->steps;
        return MBOTS_OK;
    }
    out[0] = h->sched.info_bits() | (h->S.mixed ? 16u : 0u) | (h->armed ? 32u : 0u) | (h->defer.hidden_lazy() ? 64u : 0u) |
             (h->defer.prev_action_owed() ? 128u : 0u);
    out[1] = h->sched.epoch;
    out[2] = h->sched.epoch_wraps;
    out[3] = (uint32_t)h->steps;
    return MBOTS_OK;
}

int mbots_kernel_times(mbots_handle *h, double ms[MBOTS_TK_COUNT], uint64_t launches[MBOTS_TK_COUNT])
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (h->cpu) {
        for (int k = 0; k < MBOTS_TK_COUNT; ++k) {
            if (ms) ms[k] = 0.0;
            if (launches) launches[k] = 0;
        }
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    for (auto &p : h->pending) {
        HIP_TRY(hipEventSynchronize(p.b));
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, p.a, p.b));
        h->acc_ms[p.kind] += t;
        h->acc_n[p.kind] += 1;
        h->pool.push_back(p.a);
        h->pool.push_back(p.b);
    }
    h->pending.clear();
    for (int k = 0; k < MBOTS_TK_COUNT; ++k) {
        if (ms) ms[k] = h->acc_ms[k];
        if (launches) launches[k] = h->acc_n[k];
    }
    return MBOTS_OK;
}

// ---- the trajectory window (include/mbots.h "Trajectory window") ----
int mbots_traj_open(mbots_handle *h, uint32_t horizon, uint64_t max_rows)
{
    return mbots_traj_open_ex(h, horizon, max_rows, 0u);
}

int mbots_traj_open_ex(mbots_handle *h, uint32_t horizon, uint64_t max_rows, uint32_t flags)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (flags & ~(uint32_t)(MBOTS_TRAJ_SEQ | MBOTS_TRAJ_REC_OBS | MBOTS_TRAJ_REC_STATE))
        return fail(MBOTS_E_INVALID, "unknown trajectory window flags");
    if (flags & (MBOTS_TRAJ_REC_OBS | MBOTS_TRAJ_REC_STATE)) flags |= MBOTS_TRAJ_SEQ;   // (recorded to be batched)
    if (tj.open) return fail(MBOTS_E_INVALID, "the manager already holds a trajectory window: close it first");
    if (horizon < 2 || horizon > 65535u) return fail(MBOTS_E_INVALID, "horizon must be in [2, 65535]");
    if (max_rows == 0 || max_rows >= (1ull << 31)) return fail(MBOTS_E_INVALID, "max_rows must be in [1, 2^31)");
    const uint32_t Wx = h->cfg.num_worlds;
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t col = pad((size_t)horizon * max_rows * 4), marks = pad((size_t)horizon * Wx * 4),
                 counts = pad((size_t)horizon * 4);
    // the opt-in parts follow the flagless layout, which stays as it is
    const bool seq = (flags & MBOTS_TRAJ_SEQ) != 0, rec_obs = (flags & MBOTS_TRAJ_REC_OBS) != 0,
               rec_state = (flags & MBOTS_TRAJ_REC_STATE) != 0;
    const uint32_t rec_bytes = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) ? MBOTS_ROLLOUT_BYTES_DEPTH : MBOTS_ROLLOUT_BYTES;
    const size_t slots = (size_t)horizon * max_rows;
    const size_t blks = pad(((size_t)horizon * ((max_rows + mbots::kTrajBlock - 1) / mbots::kTrajBlock) + 1) * 4),
                 recs = pad(slots * rec_bytes), hid = pad(slots * mbots::kTrajHidden * 4), masks = pad(slots);
    const size_t bytes = 8 * col + marks + counts + (seq ? 2 * col + blks : 0) + (rec_obs ? recs : 0) +
                         (rec_state ? hid + masks : 0);
    char *mem = nullptr;
    if (h->cpu) {
        mem = static_cast<char *>(std::calloc(bytes, 1));
        if (!mem) return fail(MBOTS_E_NOMEM, "host allocation of the trajectory window failed");
    } else {
        HIP_TRY(hipSetDevice(h->device));
        if (capturing_now(h)) return fail(MBOTS_E_INVALID, "a trajectory window cannot be opened under stream capture");
        if (hipMalloc((void **)&mem, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MBOTS_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for the trajectory window failed");
        }
        hipError_t e = hipMemset(mem, 0, bytes);
        if (e == hipSuccess && !tj.h_count)
            e = hipHostMalloc((void **)&tj.h_count, 65535u * sizeof(uint32_t), hipHostMallocDefault);
        if (e == hipSuccess && seq && !tj.h_S) e = hipHostMalloc((void **)&tj.h_S, sizeof(uint32_t), hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipFree(mem);
            return fail(MBOTS_E_HIP, std::string("trajectory window: ") + hipGetErrorString(e));
        }
    }
    mbots::TrajWin &w = tj.w;
    char *p = mem;
    auto take = [&](size_t b) { char *q = p; p += b; return q; };
    w.link = (int32_t *)take(col);  w.world = (int32_t *)take(col);
    w.next = (int32_t *)take(col);  w.end = (int32_t *)take(col);
    w.reward = (float *)take(col);  w.value = (float *)take(col);
    w.adv = (float *)take(col);     w.ret = (float *)take(col);
    w.mark = (int32_t *)take(marks);
    w.count = (uint32_t *)take(counts);
    w.seq_id = w.seq_pos = nullptr;
    w.blk = nullptr;
    w.rec = nullptr;
    w.hidden = nullptr;
    w.amask = nullptr;
    if (seq) {
        w.seq_id = (int32_t *)take(col);
        w.seq_pos = (int32_t *)take(col);
        w.blk = (uint32_t *)take(blks);
    }
    if (rec_obs) w.rec = (uint8_t *)take(recs);
    if (rec_state) {
        w.hidden = (float *)take(hid);
        w.amask = (uint8_t *)take(masks);
    }
    w.rec_bytes = rec_bytes;
    tj.flags = flags;
    w.horizon = horizon;
    w.max_rows = (uint32_t)max_rows;
    w.Wx = Wx;
    w.world_offset = h->cfg.world_offset;
    tj.mem = mem;
    tj.rows.assign(horizon, 0);
    tj.open = true;
    traj_empty(h);
    return MBOTS_OK;
}

int mbots_traj_close(mbots_handle *h)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (h->cpu) {
        std::free(tj.mem);
    } else {
        HIP_TRY(hipSetDevice(h->device));
        if (capturing_now(h)) return fail(MBOTS_E_INVALID, "a trajectory window cannot be closed under stream capture");
        HIP_TRY(hipDeviceSynchronize());   // its last push / compute, on whatever stream
        HIP_TRY(hipFree(tj.mem));
    }
    traj_free_extras(h);
    tj.flags = 0;
    tj.mem = nullptr;
    tj.w = mbots::TrajWin{};
    tj.open = false;
    traj_empty(h);
    return MBOTS_OK;
}

int mbots_traj_push(mbots_handle *h, const float *value, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (tj.n >= tj.w.horizon)
        return fail(MBOTS_E_INVALID, "the trajectory window is full (" + std::to_string(tj.n) +
                                         " tables): compute and clear it first");
    const uint32_t slot = mbots::traj_slot(tj.w, tj.n);
    if (h->cpu) {
        h->cpu->traj_push(tj.w, slot, value);
        const mbots::cpu::Table &t = h->cpu->table();
        const uint32_t lim = std::min<uint32_t>(h->cpu->num_agents(), tj.w.max_rows);
        if (tj.w.rec) {
            const bool fixd = (h->cfg.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
            pack_rollout_host(t.sem.data(), fixd ? t.depth.data() : nullptr, t.health.data(), t.pos.data(),
                              t.sur.data(), t.reward.data(), t.stats.data(), lim,
                              tj.w.rec + (size_t)slot * tj.w.max_rows * tj.w.rec_bytes);
        }
        if (tj.w.hidden) {
            for (uint32_t r = 0; r < lim; ++r) mbots::traj_push_mask(tj.w, slot, r, t.action.data());
            for (size_t g = 0; g < (size_t)4 * lim; ++g) mbots::traj_push_hidden(tj.w, slot, g, t.hidden.data());
        }
        tj.rows[tj.n] = tj.w.count[slot];
        tj.known = tj.n + 1;
    } else {
        HIP_TRY(hipSetDevice(h->device));
        hipStream_t st = as_stream(stream);
        Exec ex{h, st};
        if (ex.capturing())
            return fail(MBOTS_E_INVALID, "mbots_traj_push cannot be captured into a graph: the window's table count "
                                         "is host state");
        if (int rc = h->sched.enter(ex)) return rc;
        // after the step's K3a (this stream's order), which wrote the
        // provenance and the Reward column; not after its sensor
        HIP_TRY(mbots::launch_traj_push(h->S, tj.w, slot, h->T[h->defer.tb].reward, value, h->reset_mark, st));
        int rc;
        if (tj.w.hidden) {
            // Action / HiddenState where mbots_pack_learner reads them: the step's
            // deferred move of the two, then the sensor (and what it moved)
            if ((rc = h->defer.require(ex, mbots::defer::kAction | mbots::defer::kHidden, mbots::defer::How::Rows)))
                return rc;
        }
        if (tj.w.hidden || tj.w.rec) {
            if ((rc = h->sched.wait_sensor(ex))) return rc;   // the semantic / depth rows come from K3b
        }
        // (timed like mbots_pack_rollout / mbots_pack_learner: mbots_kernel_times sees them)
        if (tj.w.rec && (rc = timed(h, MBOTS_TK_OBS, st, [&] {
                return mbots::launch_pack_rollout(h->S, h->T[h->defer.tb],
                                                  tj.w.rec + (size_t)slot * tj.w.max_rows * tj.w.rec_bytes,
                                                  tj.w.max_rows, st);
            })))
            return rc;
        if (tj.w.hidden && (rc = timed(h, MBOTS_TK_OBS, st, [&] {
                return mbots::launch_traj_push_state(h->S, tj.w, slot, h->T[h->defer.tb], st);
            })))
            return rc;
    }
    ++tj.n;
    tj.computed = false;
    tj.seq_valid = false;
    return MBOTS_OK;
}

int mbots_traj_compute(mbots_handle *h, float gamma, float lambda, float death_reward, int64_t *rows_out,
                       uint32_t *n_out, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (tj.n == 0) return fail(MBOTS_E_INVALID, "the trajectory window is empty");
    hipStream_t st = as_stream(stream);
    if (!h->cpu) {
        HIP_TRY(hipSetDevice(h->device));
        Exec ex{h, st};
        if (ex.capturing())
            return fail(MBOTS_E_INVALID, "mbots_traj_compute returns the row counts to the host and cannot be "
                                         "captured into a graph");
        if (int rc = h->sched.enter(ex)) return rc;
        HIP_TRY(hipMemcpyAsync(tj.h_count, tj.w.count, (size_t)tj.w.horizon * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const uint32_t *cnt = h->cpu ? tj.w.count : tj.h_count;
    uint32_t mx = 0;
    for (uint32_t t = 0; t < tj.n; ++t) {
        const uint32_t c = cnt[mbots::traj_slot(tj.w, t)];
        tj.rows[t] = c;
        if (rows_out) rows_out[t] = c;
        mx = std::max(mx, c);
    }
    if (n_out) *n_out = tj.n;
    if (mx > tj.w.max_rows) {
        tj.known = 0;
        tj.computed = false;
        return fail(MBOTS_E_RANGE, "a pushed table held " + std::to_string(mx) + " rows, more than the window's max_rows " +
                                       std::to_string(tj.w.max_rows) + ": clear the window (or reopen it larger)");
    }
    tj.known = tj.n;
    tj.mx = mx;
    volatile float gl = gamma * lambda;   // rounded once
    const mbots::TrajParams P{gamma, gl, death_reward};
    if (h->cpu) mbots::cpu::Sim::traj_compute(tj.w, P, tj.n);
    else HIP_TRY(mbots::launch_traj_compute(tj.w, P, tj.n, mx, st));
    tj.computed = true;
    return MBOTS_OK;
}

int mbots_traj_clear(mbots_handle *h, int32_t keep_last)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (!keep_last || tj.n == 0) {
        traj_empty(h);
        return MBOTS_OK;
    }
    // the newest table's slot becomes slot of table 0: nothing moves
    const bool known = tj.known == tj.n;
    const int64_t rows_last = tj.rows[tj.n - 1];
    tj.w.base = mbots::traj_slot(tj.w, tj.n - 1);
    tj.n = 1;
    tj.rows[0] = rows_last;
    tj.known = known ? 1u : 0u;
    tj.computed = false;
    tj.seq_valid = false;
    return MBOTS_OK;
}

int mbots_traj_num_tables(mbots_handle *h, uint32_t *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    if (!h->traj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    *out = h->traj.n;
    return MBOTS_OK;
}

int mbots_traj_view(mbots_handle *h, int32_t what, uint32_t t, mbots_tensor *out)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    const mbots::TrajWin &w = tj.w;
    void *col = nullptr;
    int32_t dtype = MBOTS_DTYPE_INT32;
    bool derived = false;
    switch (what) {
    case MBOTS_TRAJ_LINK: col = w.link; break;
    case MBOTS_TRAJ_WORLD: col = w.world; break;
    case MBOTS_TRAJ_REWARD: col = w.reward; dtype = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_TRAJ_VALUE: col = w.value; dtype = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_TRAJ_NEXT: col = w.next; derived = true; break;
    case MBOTS_TRAJ_END: col = w.end; derived = true; break;
    case MBOTS_TRAJ_ADV: col = w.adv; dtype = MBOTS_DTYPE_FLOAT32; derived = true; break;
    case MBOTS_TRAJ_RET: col = w.ret; dtype = MBOTS_DTYPE_FLOAT32; derived = true; break;
    case MBOTS_TRAJ_SEQ_ID: case MBOTS_TRAJ_SEQ_POS:
        if (!w.seq_id) return fail(MBOTS_E_INVALID, "the window was opened without MBOTS_TRAJ_SEQ");
        if (t < tj.n && !tj.seq_valid)
            return fail(MBOTS_E_INVALID, "seq_id / seq_pos exist after mbots_traj_sequences of the computed tables");
        col = what == MBOTS_TRAJ_SEQ_ID ? w.seq_id : w.seq_pos;
        derived = true;
        break;
    default: return fail(MBOTS_E_INVALID, "unknown trajectory view " + std::to_string(what));
    }
    if (t >= tj.n || (what == MBOTS_TRAJ_NEXT && t + 1 >= tj.n))
        return fail(MBOTS_E_RANGE, "table " + std::to_string(t) + " is outside the window's " + std::to_string(tj.n));
    if (derived && !tj.computed)
        return fail(MBOTS_E_INVALID, "next / end / adv / ret exist after mbots_traj_compute of the pushed tables");
    if (t >= tj.known)
        return fail(MBOTS_E_INVALID, "the table's row count reaches the host with mbots_traj_compute");
    out->data = static_cast<char *>(col) + mbots::traj_at(w, t, 0) * 4;
    out->dtype = dtype;
    out->device = h->cpu ? -1 : h->device;
    out->dims[0] = tj.rows[t];
    out->dims[1] = 1;
    return MBOTS_OK;
}

int mbots_traj_sequences(mbots_handle *h, uint64_t *S_out, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (!tj.w.seq_id) return fail(MBOTS_E_INVALID, "the window was opened without MBOTS_TRAJ_SEQ");
    if (!tj.computed)
        return fail(MBOTS_E_INVALID, "mbots_traj_sequences follows an mbots_traj_compute of the tables now in the window");
    if (h->cpu) {
        tj.S = mbots::cpu::Sim::traj_sequences(tj.w, tj.n, tj.mx);
    } else {
        HIP_TRY(hipSetDevice(h->device));
        hipStream_t st = as_stream(stream);
        Exec ex{h, st};
        if (ex.capturing())
            return fail(MBOTS_E_INVALID, "mbots_traj_sequences returns the sequence count to the host and cannot be "
                                         "captured into a graph");
        if (int rc = h->sched.enter(ex)) return rc;
        HIP_TRY(mbots::launch_traj_sequences(tj.w, tj.n, tj.mx, st));
        const size_t tot = (size_t)tj.w.horizon * ((tj.w.max_rows + mbots::kTrajBlock - 1) / mbots::kTrajBlock);
        HIP_TRY(hipMemcpyAsync(tj.h_S, tj.w.blk + tot, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        tj.S = *tj.h_S;
    }
    tj.seq_valid = true;
    if (S_out) *S_out = tj.S;
    return MBOTS_OK;
}

namespace {
// the index scratch of a batch / gather: room for `entries` int32
int traj_scratch(mbots_handle *h, uint64_t entries)
{
    auto &tj = h->traj;
    if (entries <= tj.idx_cap) return MBOTS_OK;
    if (h->cpu) {
        std::free(tj.idx);
        tj.idx = static_cast<int32_t *>(std::malloc(entries * 4));
    } else {
        HIP_TRY(hipDeviceSynchronize());   // a queued batch may still read the old one
        if (tj.idx) (void)hipFree(tj.idx);
        tj.idx = nullptr;
        if (hipMalloc((void **)&tj.idx, entries * 4) != hipSuccess) {
            (void)hipGetLastError();
            tj.idx = nullptr;
        }
    }
    tj.idx_cap = tj.idx ? entries : 0;
    return tj.idx ? MBOTS_OK : fail(MBOTS_E_NOMEM, "allocation of the batch index failed");
}

// the checks mbots_traj_batch and mbots_traj_gather share; *st_out: the stream
int traj_batch_enter(mbots_handle *h, uint64_t lo, uint64_t hi, void *stream, hipStream_t *st_out)
{
    auto &tj = h->traj;
    if (!tj.open) return fail(MBOTS_E_INVALID, "no trajectory window is open");
    if (!tj.w.seq_id) return fail(MBOTS_E_INVALID, "the window was opened without MBOTS_TRAJ_SEQ");
    if (!tj.seq_valid || !tj.computed)
        return fail(MBOTS_E_INVALID, "a batch follows mbots_traj_sequences of the tables now in the window");
    if (lo > hi || hi > tj.S)
        return fail(MBOTS_E_RANGE, "sequences [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are not within [0, " +
                                       std::to_string(tj.S) + ")");
    *st_out = as_stream(stream);
    if (h->cpu) return MBOTS_OK;
    HIP_TRY(hipSetDevice(h->device));
    Exec ex{h, *st_out};
    if (ex.capturing()) return fail(MBOTS_E_INVALID, "a batch of the trajectory window cannot be captured into a graph");
    return h->sched.enter(ex);
}
}  // namespace

int mbots_traj_batch(mbots_handle *h, uint64_t lo, uint64_t hi, const struct mbots_traj_batch *out, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    auto &tj = h->traj;
    hipStream_t st = nullptr;
    if (tj.open && out->obs && !tj.w.rec)
        return fail(MBOTS_E_INVALID, "obs needs a window opened with MBOTS_TRAJ_REC_OBS");
    if (tj.open && (out->action_in || out->hidden0) && !tj.w.hidden)
        return fail(MBOTS_E_INVALID, "action_in / hidden0 need a window opened with MBOTS_TRAJ_REC_STATE");
    if (int rc = traj_batch_enter(h, lo, hi, stream, &st)) return rc;
    const uint64_t B = hi - lo;
    if (B == 0) return MBOTS_OK;
    mbots::TrajBatch o{out->rows, out->t0, out->len, out->end, out->reward, out->value,
                       out->adv,  out->ret, out->action_in, out->hidden0};
    if (out->obs && (!o.rows || !o.t0)) {   // the decode's index: the missing part in the window's scratch
        if (int rc = traj_scratch(h, (uint64_t)tj.n * B + B)) return rc;
        if (!o.rows) o.rows = tj.idx;
        if (!o.t0) o.t0 = tj.idx + (uint64_t)tj.n * B;
    }
    if (h->cpu) mbots::cpu::Sim::traj_batch(tj.w, o, (uint32_t)lo, B, tj.n, out->obs);
    else HIP_TRY(mbots::launch_traj_batch(tj.w, o, (uint32_t)lo, B, tj.n, tj.mx, out->obs, st));
    return MBOTS_OK;
}

int mbots_traj_gather(mbots_handle *h, uint64_t lo, uint64_t hi, const void *const *tables, uint32_t n_tables,
                      uint32_t row_bytes, void *out, void *stream)
{
    if (!h || !tables || !out) return fail(MBOTS_E_INVALID, "null argument");
    auto &tj = h->traj;
    hipStream_t st = nullptr;
    if (row_bytes == 0 || (row_bytes & 3u) || row_bytes > 1024u)
        return fail(MBOTS_E_INVALID, "row_bytes must be a multiple of 4 in [4, 1024]");
    if (int rc = traj_batch_enter(h, lo, hi, stream, &st)) return rc;
    if (n_tables != tj.n)
        return fail(MBOTS_E_INVALID, "mbots_traj_gather takes one table per computed table (" + std::to_string(tj.n) + ")");
    for (uint32_t t = 0; t < tj.n; ++t)
        if (!tables[t] && tj.rows[t]) return fail(MBOTS_E_INVALID, "null table");
    const uint64_t B = hi - lo;
    if (B == 0) return MBOTS_OK;
    if (int rc = traj_scratch(h, (uint64_t)tj.n * B + B)) return rc;
    mbots::TrajBatch o{};
    o.rows = tj.idx;
    o.t0 = tj.idx + (uint64_t)tj.n * B;
    if (h->cpu) {
        mbots::cpu::Sim::traj_batch(tj.w, o, (uint32_t)lo, B, tj.n, nullptr);
        mbots::cpu::Sim::traj_gather(o.rows, o.t0, B, tj.n, tables, row_bytes, out);
        return MBOTS_OK;
    }
    if (!tj.tabs || !tj.h_tabs || !tj.ev_tabs) {   // (all three, or an earlier failure left a part)
        if (!tj.tabs) HIP_TRY(hipMalloc((void **)&tj.tabs, (size_t)tj.w.horizon * sizeof(void *)));
        if (!tj.h_tabs)
            HIP_TRY(hipHostMalloc((void **)&tj.h_tabs, (size_t)tj.w.horizon * sizeof(void *), hipHostMallocDefault));
        if (!tj.ev_tabs) HIP_TRY(hipEventCreateWithFlags(&tj.ev_tabs, hipEventDisableTiming));
    } else {
        HIP_TRY(hipEventSynchronize(tj.ev_tabs));   // the last upload has left the pinned list
    }
    memcpy(tj.h_tabs, tables, (size_t)tj.n * sizeof(void *));
    HIP_TRY(hipMemcpyAsync(tj.tabs, tj.h_tabs, (size_t)tj.n * sizeof(void *), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(tj.ev_tabs, st));
    HIP_TRY(mbots::launch_traj_batch(tj.w, o, (uint32_t)lo, B, tj.n, tj.mx, nullptr, st));
    HIP_TRY(mbots::launch_traj_gather(o.rows, o.t0, B, tj.n, tj.tabs, row_bytes, out, st));
    return MBOTS_OK;
}

// ---- the device actor (include/mbots.h "Acting on the device") ----
// the layers of a net in upload order: trunk, actor, critic, memory, gate
static std::vector<mbots::PolLayer *> policy_layers(mbots::PolNet &n)
{
    std::vector<mbots::PolLayer *> v;
    for (uint32_t l = 0; l < n.n_trunk; ++l) v.push_back(&n.trunk[l]);
    v.push_back(&n.actor[0]);
    v.push_back(&n.actor[1]);
    v.push_back(&n.critic[0]);
    v.push_back(&n.critic[1]);
    if (n.has_memory) v.push_back(&n.memory);
    if (n.gated) v.push_back(&n.gate);
    return v;
}

// the widths of `src` checked and laid out (no storage yet)
static int policy_describe(const mbots_policy_net *src, mbots::PolNet &n)
{
    using namespace mbots;
    n = PolNet{};
    if (src->n_trunk < 1 || src->n_trunk > (uint32_t)kPolMaxTrunk)
        return fail(MBOTS_E_INVALID, "a policy net has 1..4 trunk layers");
    if (src->flags & ~(MBOTS_POLICY_MEMORY_IN | MBOTS_POLICY_GATE))
        return fail(MBOTS_E_INVALID, "unknown policy net flags");
    const uint32_t H = src->trunk[0].out, in0 = (src->flags & MBOTS_POLICY_MEMORY_IN) ? kPolObs + kHidden : kPolObs;
    if (H < 16 || H > (uint32_t)kPolMaxH || H % 16u)
        return fail(MBOTS_E_INVALID, "the trunk width must be a multiple of 16 in [16, 128], not " + std::to_string(H));
    auto lay = [&](const mbots_policy_layer &s, PolLayer &d, uint32_t in, uint32_t out, const char *what) {
        if (s.in != in || s.out != out)
            return fail(MBOTS_E_INVALID, std::string(what) + " must be Linear(" + std::to_string(in) + ", " +
                                             std::to_string(out) + "), not (" + std::to_string(s.in) + ", " +
                                             std::to_string(s.out) + ")");
        if (!s.weight) return fail(MBOTS_E_INVALID, std::string(what) + ": null weight");
        d.in = in;
        d.out = out;
        d.kp = pol_kp(in);
        d.nt = (out + 15u) / 16u;
        d.act = 0;
        return MBOTS_OK;
    };
    n.n_trunk = src->n_trunk;
    n.H = H;
    n.flags = src->flags;
    n.has_memory = src->memory.weight ? 1u : 0u;
    for (uint32_t l = 0; l < n.n_trunk; ++l) {
        if (int rc = lay(src->trunk[l], n.trunk[l], l ? H : in0, H, "a trunk layer")) return rc;
        if (src->trunk[l].act < 0 || src->trunk[l].act > kActLogSigmoid)
            return fail(MBOTS_E_INVALID, "unknown activation code " + std::to_string(src->trunk[l].act));
        n.trunk[l].act = (uint32_t)src->trunk[l].act;
    }
    if (int rc = lay(src->actor[0], n.actor[0], H, H, "the actor's first layer")) return rc;
    if (int rc = lay(src->actor[1], n.actor[1], H, kPolActions, "the actor's second layer")) return rc;
    if (int rc = lay(src->critic[0], n.critic[0], H, H, "the critic's first layer")) return rc;
    if (int rc = lay(src->critic[1], n.critic[1], H, 1, "the critic's second layer")) return rc;
    if (n.has_memory)
        if (int rc = lay(src->memory, n.memory, H, kHidden, "the memory head")) return rc;
    // (src->gate is read under the flag alone: a caller that never sets it may
    // have built against the struct without the field)
    if (src->flags & MBOTS_POLICY_GATE) {
        if (!n.has_memory)
            return fail(MBOTS_E_INVALID, "MBOTS_POLICY_GATE: a gate head blends the memory head's output into "
                                         "HiddenState, and the net has no memory head");
        if (!(src->flags & MBOTS_POLICY_MEMORY_IN))
            return fail(MBOTS_E_INVALID, "MBOTS_POLICY_GATE: a gated net reads the HiddenState it blends "
                                         "(MBOTS_POLICY_MEMORY_IN)");
        if (int rc = lay(src->gate, n.gate, H, kHidden, "the gate head")) return rc;
        n.gated = 1;
    }
    n.set = 1;
    return MBOTS_OK;
}

// the CPU mode's copy of one layer: [nt * 16][kp] rows and the bias, +0 pads
static void policy_fill_host(const mbots::PolLayer &d, const mbots_policy_layer &s)
{
    for (uint32_t j = 0; j < d.nt * 16u; ++j) {
        for (uint32_t k = 0; k < d.kp; ++k)
            d.w[(size_t)j * d.kp + k] = (j < d.out && k < d.in) ? s.weight[(size_t)j * d.in + k] : 0.0f;
        d.b[j] = (j < d.out && s.bias) ? s.bias[j] : 0.0f;
    }
}

static bool policy_same_arch(mbots::PolNet &a, mbots::PolNet &b)
{
    if (!a.set || !b.set || a.n_trunk != b.n_trunk || a.H != b.H || a.flags != b.flags || a.has_memory != b.has_memory ||
        a.gated != b.gated)
        return false;
    for (uint32_t l = 0; l < a.n_trunk; ++l)
        if (a.trunk[l].in != b.trunk[l].in || a.trunk[l].act != b.trunk[l].act) return false;
    return true;
}

// the groups as the kernels and the CPU loops take them (mbots_policy.hpp)
static mbots::PolGroups policy_groups_view(const mbots_handle *h)
{
    mbots::PolGroups g{};
    const std::vector<uint32_t> &st = h->pol.starts;
    const uint32_t G = h->pol.groups(), off = h->cfg.world_offset, Wx = h->cfg.num_worlds;
    g.table = h->cpu ? h->pol.nets.data() : h->pol.table;
    g.G = G;
    for (uint32_t i = 0; i < G; ++i) g.first[i] = st[i] <= off ? 0u : std::min(st[i] - off, Wx);
    g.first[G] = Wx;
    g.ghost = mbots::pol_group_of(st.data(), G, off + Wx);
    return g;
}

// does group g own one of the manager's worlds (the shard ghost's included)?
static bool policy_group_needed(const mbots_handle *h, uint32_t g)
{
    const std::vector<uint32_t> &st = h->pol.starts;
    const uint64_t lo = h->cfg.world_offset;
    const uint64_t hi = lo + h->cfg.num_worlds + ((h->cfg.flags & MBOTS_FLAG_SHARD_GHOST) ? 1u : 0u);
    return st[g] < hi && (g + 1u == st.size() || st[g + 1u] > lo);
}

static int policy_set_one(mbots_handle *h, uint32_t group, uint32_t species, const struct mbots_policy_net *net,
                          void *stream)
{
    using namespace mbots;
    PolNet n;
    if (int rc = policy_describe(net, n)) return rc;
    const size_t slot = (size_t)group * kNumSpecies + (species - 1);
    PolNet &cur = h->pol.nets[slot];
    hipStream_t st = nullptr;
    if (!h->cpu) {
        HIP_TRY(hipSetDevice(h->device));
        st = as_stream(stream);
        Exec ex{h, st};
        if (int rc = h->sched.enter(ex)) return rc;
    }
    std::vector<PolLayer *> L = policy_layers(n);
    if (!policy_same_arch(cur, n)) {
        size_t floats = 0;
        for (PolLayer *l : L) floats += ((pol_w_floats(*l) + 63u) & ~size_t(63)) + ((pol_b_floats(*l) + 63u) & ~size_t(63));
        float *mem = nullptr;
        if (h->cpu) {
            mem = static_cast<float *>(std::malloc(floats * sizeof(float)));
            if (!mem) return fail(MBOTS_E_NOMEM, "policy net allocation failed");
            std::free(h->pol.mem[slot]);
        } else {
            if (capturing(h, st))
                return fail(MBOTS_E_INVALID, "a policy net of a new architecture allocates: set it before the capture "
                                             "begins (a net of the same architecture is re-uploaded in place)");
            HIP_TRY(hipDeviceSynchronize());   // a queued act may still read the net in place
            if (!h->pol.draw) {
                HIP_TRY(hipMalloc((void **)&h->pol.draw, 256));
                HIP_TRY(hipMemset(h->pol.draw, 0, 256));
            }
            if (hipMalloc((void **)&mem, floats * sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(MBOTS_E_NOMEM, "policy net allocation failed");
            }
            if (h->pol.mem[slot]) (void)hipFree(h->pol.mem[slot]);
        }
        h->pol.mem[slot] = mem;
        for (PolLayer *l : L) {
            l->w = mem;
            mem += (pol_w_floats(*l) + 63u) & ~size_t(63);
            l->b = mem;
            mem += (pol_b_floats(*l) + 63u) & ~size_t(63);
        }
        cur = n;
        // (the device has drained: the table's entry changes only here and in a
        // clear, never under a capture; a re-upload leaves it as it is)
        if (h->pol.table) HIP_TRY(hipMemcpy(h->pol.table + slot, &cur, sizeof(PolNet), hipMemcpyHostToDevice));
    }
    // the weights into the storage in place
    std::vector<PolLayer *> D = policy_layers(cur);
    std::vector<const mbots_policy_layer *> S;
    for (uint32_t l = 0; l < net->n_trunk; ++l) S.push_back(&net->trunk[l]);
    S.push_back(&net->actor[0]);
    S.push_back(&net->actor[1]);
    S.push_back(&net->critic[0]);
    S.push_back(&net->critic[1]);
    if (cur.has_memory) S.push_back(&net->memory);
    if (cur.gated) S.push_back(&net->gate);
    if (h->cpu) {
        for (size_t i = 0; i < D.size(); ++i) policy_fill_host(*D[i], *S[i]);
        return MBOTS_OK;
    }
    PolUploads U{};
    for (size_t i = 0; i < D.size(); ++i) {
        const PolLayer &d = *D[i];
        U.l[i] = PolUpload{S[i]->weight, S[i]->bias, d.w, d.b, d.in, d.out, d.kp, d.nt};
    }
    U.n = (uint32_t)D.size();
    HIP_TRY(launch_policy_repack(U, st));
    return MBOTS_OK;
}

static int policy_clear_one(mbots_handle *h, uint32_t group, uint32_t species)
{
    const size_t slot = (size_t)group * mbots::kNumSpecies + (species - 1);
    if (!h->pol.mem[slot]) return MBOTS_OK;   // no net there: nothing to wait for, nothing to write
    if (h->cpu) {
        std::free(h->pol.mem[slot]);
    } else {
        HIP_TRY(hipSetDevice(h->device));
        if (capturing_now(h)) return fail(MBOTS_E_INVALID, "a policy net cannot be cleared during a graph capture");
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(h->pol.mem[slot]);
    }
    h->pol.mem[slot] = nullptr;
    h->pol.nets[slot] = mbots::PolNet{};
    if (h->pol.table)
        HIP_TRY(hipMemcpy(h->pol.table + slot, &h->pol.nets[slot], sizeof(mbots::PolNet), hipMemcpyHostToDevice));
    return MBOTS_OK;
}

static int policy_check_group(mbots_handle *h, uint32_t group, uint32_t species)
{
    if (species < 1 || species > (uint32_t)mbots::kNumSpecies) return fail(MBOTS_E_INVALID, "species must be 1..4");
    if (group >= h->pol.groups())
        return fail(MBOTS_E_INVALID, "policy group " + std::to_string(group) + " out of range: the manager has " +
                                         std::to_string(h->pol.groups()) + " (mbots_policy_groups)");
    return MBOTS_OK;
}

int mbots_policy_set(mbots_handle *h, uint32_t species, const struct mbots_policy_net *net, void *stream)
{
    if (!h || !net) return fail(MBOTS_E_INVALID, "null argument");
    if (species < 1 || species > (uint32_t)mbots::kNumSpecies) return fail(MBOTS_E_INVALID, "species must be 1..4");
    for (uint32_t g = 0; g < h->pol.groups(); ++g)
        if (int rc = policy_set_one(h, g, species, net, stream)) return rc;
    return MBOTS_OK;
}

int mbots_policy_set_group(mbots_handle *h, uint32_t group, uint32_t species, const struct mbots_policy_net *net,
                           void *stream)
{
    if (!h || !net) return fail(MBOTS_E_INVALID, "null argument");
    if (int rc = policy_check_group(h, group, species)) return rc;
    return policy_set_one(h, group, species, net, stream);
}

int mbots_policy_clear(mbots_handle *h, uint32_t species)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (species < 1 || species > (uint32_t)mbots::kNumSpecies) return fail(MBOTS_E_INVALID, "species must be 1..4");
    for (uint32_t g = 0; g < h->pol.groups(); ++g)
        if (int rc = policy_clear_one(h, g, species)) return rc;
    return MBOTS_OK;
}

int mbots_policy_clear_group(mbots_handle *h, uint32_t group, uint32_t species)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (int rc = policy_check_group(h, group, species)) return rc;
    return policy_clear_one(h, group, species);
}

int mbots_policy_groups(mbots_handle *h, const uint32_t *starts, uint32_t n)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    static const uint32_t kOne[1] = {0u};
    if (!starts || n == 0) {
        starts = kOne;
        n = 1;
    }
    if (n > (uint32_t)MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, std::to_string(n) + " policy groups: at most " +
                                         std::to_string(MBOTS_POLICY_MAX_GROUPS) + " (MBOTS_POLICY_MAX_GROUPS)");
    if (starts[0] != 0u)
        return fail(MBOTS_E_INVALID, "policy group starts begin at world 0, not " + std::to_string(starts[0]));
    for (uint32_t i = 1; i < n; ++i)
        if (starts[i] <= starts[i - 1])
            return fail(MBOTS_E_INVALID, "policy group starts must be ascending: starts[" + std::to_string(i) + "] = " +
                                             std::to_string(starts[i]) + " after " + std::to_string(starts[i - 1]));
    if (std::vector<uint32_t>(starts, starts + n) == h->pol.starts) return MBOTS_OK;
    if (!h->cpu) {
        HIP_TRY(hipSetDevice(h->device));
        if (capturing_now(h))
            return fail(MBOTS_E_INVALID, "policy groups cannot be changed during a graph capture");
        HIP_TRY(hipDeviceSynchronize());   // a queued act may still read the nets and the table in place
        if (n > 1 && !h->pol.table) {
            const size_t bytes = (size_t)MBOTS_POLICY_MAX_GROUPS * mbots::kNumSpecies * sizeof(mbots::PolNet);
            if (hipMalloc((void **)&h->pol.table, bytes) != hipSuccess) {
                (void)hipGetLastError();
                h->pol.table = nullptr;
                return fail(MBOTS_E_NOMEM, "policy net table allocation failed");
            }
        }
        if (h->pol.table)
            HIP_TRY(hipMemset(h->pol.table, 0,
                              (size_t)MBOTS_POLICY_MAX_GROUPS * mbots::kNumSpecies * sizeof(mbots::PolNet)));
    }
    // every net goes with the old groups
    for (float *&p : h->pol.mem) {
        if (h->cpu) std::free(p);
        else if (p) (void)hipFree(p);
        p = nullptr;
    }
    h->pol.starts.assign(starts, starts + n);
    h->pol.nets.assign((size_t)n * mbots::kNumSpecies, mbots::PolNet{});
    h->pol.mem.assign((size_t)n * mbots::kNumSpecies, nullptr);
    return MBOTS_OK;
}

int mbots_policy_num_groups(mbots_handle *h, uint32_t *n, uint32_t *starts_out)
{
    if (!h || !n) return fail(MBOTS_E_INVALID, "null argument");
    *n = h->pol.groups();
    if (starts_out) std::copy(h->pol.starts.begin(), h->pol.starts.end(), starts_out);
    return MBOTS_OK;
}

int mbots_policy_segments(mbots_handle *h, int32_t *out, void *stream)
{
    if (!h || !out) return fail(MBOTS_E_INVALID, "null argument");
    const mbots::PolGroups G = policy_groups_view(h);
    if (h->cpu) {
        h->cpu->policy_segments(G, out);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    if (int rc = h->sched.enter(ex)) return rc;
    HIP_TRY(mbots::launch_policy_segments(h->S, G, out, st));
    return MBOTS_OK;
}

int mbots_policy_act(mbots_handle *h, uint32_t flags, int32_t *action_out, float *logp_out, float *value_out,
                     uint64_t out_rows, void *stream)
{
    if (!h) return fail(MBOTS_E_INVALID, "null handle");
    if (flags & ~(MBOTS_ACT_GREEDY | MBOTS_ACT_NO_WRITE)) return fail(MBOTS_E_INVALID, "unknown act flags");
    // the nets of every (group, species) that owns one of the manager's worlds,
    // and what they do with HiddenState
    const uint32_t nG = h->pol.groups();
    bool writes_hidden = false, reads_hidden = false, all_hidden = true, any_gated = false;
    for (uint32_t g = 0; g < nG; ++g) {
        if (!policy_group_needed(h, g)) continue;
        for (int s = 0; s < mbots::kNumSpecies; ++s) {
            const mbots::PolNet &n = h->pol.nets[(size_t)g * mbots::kNumSpecies + s];
            if (!n.set)
                return fail(MBOTS_E_INVALID, (nG > 1 ? "group " + std::to_string(g) + " species " : std::string("species ")) +
                                                 std::to_string(s + 1) + " has no policy net (mbots_policy_set)");
            writes_hidden |= n.has_memory != 0;
            all_hidden &= n.has_memory != 0;
            reads_hidden |= (n.flags & mbots::kPolMemoryIn) != 0u;
            any_gated |= n.gated != 0u;
        }
    }
    if (out_rows > 0xFFFFFFFFull) out_rows = 0xFFFFFFFFull;
    const mbots::PolGroups G = policy_groups_view(h);
    if (h->cpu) {
        h->cpu->policy_act(G, flags, h->pol.draw_host, action_out, logp_out, value_out, out_rows);
        h->pol.draw_host += 1u;
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = as_stream(stream);
    Exec ex{h, st};
    int rc = h->sched.enter(ex);
    if (rc) return rc;
    const int tb = h->defer.tb;
    namespace defer = mbots::defer;
    // the inputs: the sensor's rows (mbots_construct_obs), and HiddenState where
    // its readers find it (the step's deferred move done; a column a fused shift
    // left aliased is read in its Prev storage, not copied)
    if ((rc = h->sched.wait_sensor(ex))) return rc;
    // (a lazy HiddenState column a net reads, or keeps rows of: real rows first;
    // memoryless nets leave it lazy)
    if ((rc = h->defer.require(ex, defer::kAction | (reads_hidden || writes_hidden ? defer::kHidden : 0),
                               defer::How::View)))
        return rc;
    const bool write = !(flags & MBOTS_ACT_NO_WRITE);
    // a net without a memory head leaves its rows' HiddenState as it is: if the
    // column is written at all (another net's head) while still aliased, the
    // rows it keeps are copied out first, as mbots_write_actions does for a part
    if (write && writes_hidden && !all_hidden && (rc = h->defer.require(ex, defer::kHidden, defer::How::WritePart)))
        return rc;
    const float *hidden_in = src_view(h, tb).hidden;
    // (the columns the nets write whole are simply written)
    if (write && (rc = h->defer.require(ex, defer::kAction | (writes_hidden ? defer::kHidden : 0), defer::How::WriteAll)))
        return rc;
    // one group: its four nets by value, as ever; more: the table in device memory
    mbots::PolNets four{};
    if (nG == 1)
        for (int s = 0; s < mbots::kNumSpecies; ++s) four.net[s] = h->pol.nets[s];
    rc = timed(h, MBOTS_TK_ACTIONS, st, [&] {
        return mbots::launch_policy_act(h->S, h->T[tb], hidden_in, four, nG > 1 ? &G : nullptr, any_gated, flags,
                                        h->pol.draw,
                                        action_out, logp_out, value_out, (uint32_t)out_rows,
                                        (uint32_t)((uint64_t)h->S.W * h->S.cap), st);
    });
    if (rc) return rc;
    HIP_TRY(mbots::launch_policy_draw_next(h->pol.draw, st));
    return MBOTS_OK;
}

int mbots_policy_draw(mbots_handle *h, int32_t set, uint32_t *value)
{
    if (!h || !value) return fail(MBOTS_E_INVALID, "null argument");
    if (h->cpu) {
        if (set) h->pol.draw_host = *value;
        else *value = h->pol.draw_host;
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (capturing_now(h)) return fail(MBOTS_E_INVALID, "the draw counter cannot be read or set during a graph capture");
    if (!h->pol.draw) {
        HIP_TRY(hipMalloc((void **)&h->pol.draw, 256));
        HIP_TRY(hipMemset(h->pol.draw, 0, 256));
    }
    if (set) {
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->pol.draw, (int)*value, 1, last_stream(h)));
        return MBOTS_OK;
    }
    HIP_TRY(hipMemcpyAsync(value, h->pol.draw, sizeof(uint32_t), hipMemcpyDeviceToHost, last_stream(h)));
    HIP_TRY(hipStreamSynchronize(last_stream(h)));
    return MBOTS_OK;
}

int mbots_policy_activation(int32_t act, const float *x, float *y, uint64_t n, int32_t device, void *stream)
{
    if ((!x || !y) && n) return fail(MBOTS_E_INVALID, "null argument");
    if (act < 0 || act > mbots::kActSigmoid) return fail(MBOTS_E_INVALID, "unknown activation code " + std::to_string(act));
    if (device < 0) {
        for (uint64_t i = 0; i < n; ++i) y[i] = mbots::pol_activation_any(act, x[i]);
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_policy_activation(act, x, y, n, as_stream(stream)));
    return MBOTS_OK;
}

// ---- evaluate and its backward pass (include/mbots.h "Learning from what the
// actor did") ----
namespace {
// where a call's pieces lie in the caller's workspace
struct EvalPlan {
    mbots::PolNet net, back;                  // w / b point into the workspace once bound
    const mbots_policy_layer *src[mbots::kPolGateLayers];
    mbots::PolLayer *fwd[mbots::kPolGateLayers], *bwd[mbots::kPolGateLayers];   // null: no such layer
    mbots::PolGradSlabs slabs;                // base bound; the device's layout, or the CPU mode's
    mbots::PolGradOut out;
    // the slice of src's weight a back layer transposes: its row stride (0: the
    // layer's own width) and first column
    uint32_t bwd_ld[mbots::kPolGateLayers], bwd_off[mbots::kPolGateLayers];
    size_t stash_off, h_off, floats;
};

// what a plan is laid out for: evaluate over n rows, or evaluate_sequences over
// n sequences of L steps
struct EvalMode {
    bool seq;
    uint32_t L;   // (seq only)
};
constexpr EvalMode kEvalRows{false, 0u};

// With mode.seq the memory head takes part (slot kPolGradLayers), bwd[0] is the
// H -> 16 layer over the first layer's HiddenState columns, and the workspace
// ends with the accumulators' h_k store; without, the layout is evaluate's.  A
// gated net's gate head follows the memory head (slot kPolSeqLayers).
int eval_plan(const mbots_policy_net *src, uint64_t n, bool cpu, float *ws, EvalPlan &P, EvalMode mode)
{
    using namespace mbots;
    const bool seq = mode.seq;
    if (int rc = policy_describe(src, P.net)) return rc;
    if (seq && !(P.net.has_memory && (P.net.flags & kPolMemoryIn)))
        return fail(MBOTS_E_INVALID, "sequences are evaluated by a net with a memory head and MBOTS_POLICY_MEMORY_IN "
                                     "(a net without them has no state to carry: mbots_policy_eval)");
    if (!seq) P.net.has_memory = 0, P.net.gated = 0;   // evaluate ignores both heads
    P.back = PolNet{};
    const uint32_t T = P.net.n_trunk;
    for (int i = 0; i < kPolGateLayers; ++i)
        P.src[i] = nullptr, P.fwd[i] = nullptr, P.bwd[i] = nullptr, P.bwd_ld[i] = 0u, P.bwd_off[i] = 0u;
    if (seq) {
        P.bwd[0] = &P.back.trunk[0];
        P.src[kPolGradLayers] = &src->memory;
        P.fwd[kPolGradLayers] = &P.net.memory;
        P.bwd[kPolGradLayers] = &P.back.memory;
        if (P.net.gated) {
            P.src[kPolSeqLayers] = &src->gate;
            P.fwd[kPolSeqLayers] = &P.net.gate;
            P.bwd[kPolSeqLayers] = &P.back.gate;
        }
    }
    for (uint32_t l = 0; l < T; ++l) {
        P.src[l] = &src->trunk[l];
        P.fwd[l] = &P.net.trunk[l];
        if (l) P.bwd[l] = &P.back.trunk[l];
    }
    for (int i = 0; i < 2; ++i) {
        P.src[kPolMaxTrunk + i] = &src->actor[i];
        P.fwd[kPolMaxTrunk + i] = &P.net.actor[i];
        P.bwd[kPolMaxTrunk + i] = &P.back.actor[i];
        P.src[kPolMaxTrunk + 2 + i] = &src->critic[i];
        P.fwd[kPolMaxTrunk + 2 + i] = &P.net.critic[i];
        P.bwd[kPolMaxTrunk + 2 + i] = &P.back.critic[i];
    }
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = ws ? ws + off : nullptr;
        off += (floats + 63u) & ~size_t(63);
        return p;
    };
    const uint64_t tiles = (n + kPolGradRows - 1u) / kPolGradRows;
    P.slabs = PolGradSlabs{};
    P.slabs.nacc = (uint32_t)std::min<uint64_t>(tiles, kPolGradAcc);
    P.out = PolGradOut{};
    P.out.n = seq ? (P.net.gated ? kPolGateLayers : kPolSeqLayers) : kPolGradLayers;
    size_t slab = 0, slab_cpu = 0;
    for (int i = 0; i < (int)P.out.n; ++i) {
        if (!P.fwd[i]) continue;
        PolLayer &f = *P.fwd[i];
        f.w = take(pol_w_floats(f));
        f.b = take(pol_b_floats(f));
        if (P.bwd[i]) {
            PolLayer &b = *P.bwd[i];
            b.in = f.out;
            b.out = f.in;
            if (i == 0) {   // W0[:, 69:85] alone: dh_k
                b.out = (uint32_t)kHidden;
                P.bwd_ld[i] = f.in;
                P.bwd_off[i] = (uint32_t)kPolObs;
            }
            b.kp = (b.in + 7u) & ~7u;   // an even number of k-steps, as the layer kernel's paired loop takes
            b.nt = (b.out + 15u) / 16u;
            b.w = take(pol_w_floats(b));
            b.b = take(pol_b_floats(b));
        }
        P.out.in[i] = f.in;
        P.out.out[i] = f.out;
        P.out.kp[i] = f.kp;
        // (the CPU mode's [out][in] slab is never larger than the device's tiles)
        P.slabs.w[i] = (uint32_t)(cpu ? slab_cpu : slab);
        slab += (size_t)f.nt * pol_grad_nkt(f.kp) * 256u;
        slab_cpu += (size_t)f.out * f.in;
        P.slabs.b[i] = (uint32_t)(cpu ? slab_cpu : slab);
        slab += (size_t)f.nt * 16u;
        slab_cpu += f.out;
    }
    P.slabs.slab_floats = cpu ? slab_cpu : slab;
    P.slabs.base = take(slab * P.slabs.nacc);
    P.stash_off = off;
    take(policy_grad_stash_floats(P.slabs.nacc));
    P.h_off = off;
    if (seq) take(pol_seq_h_floats(P.slabs.nacc, mode.L));
    P.floats = off;
    return MBOTS_OK;
}

int eval_check(const mbots_policy_net *net, const float *obs, const float *hidden, const int32_t *action, uint64_t n,
               void *ws, uint64_t ws_bytes, int32_t device, EvalPlan &P)
{
    if (!net) return fail(MBOTS_E_INVALID, "null argument");
    if (int rc = eval_plan(net, n, device < 0, static_cast<float *>(ws), P, kEvalRows)) return rc;
    if (n && (!obs || !action)) return fail(MBOTS_E_INVALID, "null obs or action");
    if (n && (net->flags & MBOTS_POLICY_MEMORY_IN) && !hidden)
        return fail(MBOTS_E_INVALID, "a net with MBOTS_POLICY_MEMORY_IN needs the rows' hidden floats");
    if (!ws || ((uintptr_t)ws & 15u)) return fail(MBOTS_E_INVALID, "the workspace must be 16-byte aligned memory");
    if (ws_bytes < P.floats * sizeof(float))
        return fail(MBOTS_E_INVALID, "workspace of " + std::to_string(ws_bytes) + " bytes, " +
                                         std::to_string(P.floats * sizeof(float)) + " needed (mbots_policy_grad_workspace)");
    if (device < 0)
        for (uint64_t r = 0; r < n; ++r)
            if (action[r] < 0 || action[r] >= mbots::kPolActions)
                return fail(MBOTS_E_INVALID, "action " + std::to_string(action[r]) + " of row " + std::to_string(r) +
                                                 " is outside 0..5");
    return MBOTS_OK;
}

// the weights into the workspace: fragment order on the device (the transposed
// layers too when `back`), the CPU mode's rows on the host
int eval_upload(const EvalPlan &P, bool back, int32_t device, hipStream_t st)
{
    using namespace mbots;
    PolUploads U{}, B{};
    for (int i = 0; i < (int)P.out.n; ++i) {
        if (!P.fwd[i]) continue;
        const PolLayer &f = *P.fwd[i];
        if (device < 0) {
            policy_fill_host(f, *P.src[i]);
            continue;
        }
        U.l[U.n++] = PolUpload{P.src[i]->weight, P.src[i]->bias, f.w, f.b, f.in, f.out, f.kp, f.nt, 0u};
        if (back && P.bwd[i]) {
            const PolLayer &b = *P.bwd[i];
            B.l[B.n++] = PolUpload{P.src[i]->weight, nullptr, b.w, b.b, b.in, b.out, b.kp, b.nt, 1u, P.bwd_ld[i],
                                   P.bwd_off[i]};
        }
    }
    if (device < 0) return MBOTS_OK;
    HIP_TRY(launch_policy_repack(U, st));
    HIP_TRY(launch_policy_repack(B, st));
    return MBOTS_OK;
}
}  // namespace

int mbots_policy_grad_workspace(const struct mbots_policy_net *net, uint64_t n, uint64_t *bytes)
{
    if (!net || !bytes) return fail(MBOTS_E_INVALID, "null argument");
    EvalPlan P;
    if (int rc = eval_plan(net, n, false, nullptr, P, kEvalRows)) return rc;
    *bytes = P.floats * sizeof(float);
    return MBOTS_OK;
}

int mbots_policy_eval(const struct mbots_policy_net *net, const float *obs, const float *hidden,
                      const int32_t *action, uint64_t n, float *logp, float *value, float *entropy, void *workspace,
                      uint64_t workspace_bytes, int32_t device, void *stream)
{
    EvalPlan P;
    if (int rc = eval_check(net, obs, hidden, action, n, workspace, workspace_bytes, device, P)) return rc;
    const mbots::PolEvalIO io{obs, hidden, action, nullptr, nullptr, nullptr, logp, value, entropy, n};
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = eval_upload(P, false, device, as_stream(stream))) return rc;
    if (device < 0) {
        mbots::cpu::policy_eval(P.net, io);
        return MBOTS_OK;
    }
    HIP_TRY(mbots::launch_policy_eval(io, P.net, as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_grad(const struct mbots_policy_net *net, const float *obs, const float *hidden,
                      const int32_t *action, uint64_t n, const float *g_logp, const float *g_value,
                      const float *g_entropy, const struct mbots_policy_grads *out, void *workspace,
                      uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (!out) return fail(MBOTS_E_INVALID, "null argument");
    EvalPlan P;
    if (int rc = eval_check(net, obs, hidden, action, n, workspace, workspace_bytes, device, P)) return rc;
    for (uint32_t l = 0; l < P.net.n_trunk; ++l) P.out.w[l] = out->trunk[l].weight, P.out.b[l] = out->trunk[l].bias;
    for (int i = 0; i < 2; ++i) {
        P.out.w[kPolMaxTrunk + i] = out->actor[i].weight;
        P.out.b[kPolMaxTrunk + i] = out->actor[i].bias;
        P.out.w[kPolMaxTrunk + 2 + i] = out->critic[i].weight;
        P.out.b[kPolMaxTrunk + 2 + i] = out->critic[i].bias;
    }
    const PolEvalIO io{obs, hidden, action, g_logp, g_value, g_entropy, nullptr, nullptr, nullptr, n};
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = eval_upload(P, true, device, as_stream(stream))) return rc;
    if (device < 0) {
        cpu::policy_grad(P.net, io, P.slabs, P.out);
        return MBOTS_OK;
    }
    HIP_TRY(launch_policy_grad(io, P.net, P.back, P.slabs, static_cast<float *>(workspace) + P.stash_off, P.out,
                               as_stream(stream)));
    return MBOTS_OK;
}

// ---- grouped evaluate (include/mbots.h "Every group's nets in one call") ----
namespace {
// where a grouped call's pieces lie in the caller's workspace (floats): the
// descriptor table, the repack list, every net's packed weights, and one
// wave's slabs and stash
struct GroupsPlan {
    std::vector<mbots::PolGroupSpec> spec;   // [4 groups]; n_trunk == 0: no net
    std::vector<uint32_t> present;           // the segments that have one
    bool memory_in = false;
    size_t table_off = 0, upload_off = 0, slab_off = 0, stash_off = 0, floats = 0;
    uint64_t slab_stride = 0;
    uint32_t wave_acc = 0;                   // accumulators of a segment at most: min(256, tiles of n rows)
};

// "group g species s" of segment e, as mbots_policy_act names a pair
const auto pair_name = [](uint32_t e) {
    return "group " + std::to_string(e >> 2) + " species " + std::to_string((e & 3u) + 1u);
};
int fail_pair(int rc, uint32_t e) { return fail(rc, pair_name(e) + ": " + g_err); }

int groups_plan(const mbots_policy_net *nets, uint32_t groups, uint64_t n, GroupsPlan &P)
{
    using namespace mbots;
    if (!nets) return fail(MBOTS_E_INVALID, "null nets");
    if (groups < 1 || groups > kPolMaxGroups)
        return fail(MBOTS_E_INVALID, "1.." + std::to_string(kPolMaxGroups) + " groups, not " + std::to_string(groups));
    if (n > 0x7FFFFFFFull) return fail(MBOTS_E_INVALID, "segments address rows as int32: at most 2^31 - 1 rows");
    const uint32_t nseg = 4u * groups;
    P.spec.assign(nseg, PolGroupSpec{});
    size_t off = 0, cpu_floats = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 63u) & ~size_t(63);
        return at;
    };
    P.table_off = take((size_t)nseg * sizeof(PolGroupEntry) / sizeof(float));
    P.upload_off = take((size_t)nseg * kPolGroupUploads * sizeof(PolUpload) / sizeof(float));
    for (uint32_t e = 0; e < nseg; ++e) {
        const mbots_policy_net &src = nets[e];
        if (src.n_trunk == 0) continue;
        PolNet d;
        if (int rc = policy_describe(&src, d)) return fail_pair(rc, e);
        PolGroupSpec &s = P.spec[e];
        s.w_off = off;
        s.n_trunk = d.n_trunk;
        s.H = d.H;
        s.flags = d.flags;
        for (uint32_t l = 0; l < d.n_trunk; ++l) {
            s.act |= d.trunk[l].act << (8u * l);
            s.w[l] = src.trunk[l].weight, s.b[l] = src.trunk[l].bias;
        }
        for (int i = 0; i < 2; ++i) {
            s.w[kPolMaxTrunk + i] = src.actor[i].weight, s.b[kPolMaxTrunk + i] = src.actor[i].bias;
            s.w[kPolMaxTrunk + 2 + i] = src.critic[i].weight, s.b[kPolMaxTrunk + 2 + i] = src.critic[i].bias;
        }
        PolGroupEntry E;
        off += pol_group_entry(s, nullptr, E, nullptr);
        P.slab_stride = std::max<uint64_t>(P.slab_stride, E.slab_floats);
        P.memory_in |= (d.flags & kPolMemoryIn) != 0u;
        P.present.push_back(e);
        // (the host path runs evaluate's own plan, one net at a time, in the same memory)
        EvalPlan one;
        if (int rc = eval_plan(&src, n, true, nullptr, one, kEvalRows)) return fail_pair(rc, e);
        cpu_floats = std::max(cpu_floats, one.floats);
    }
    P.wave_acc = (uint32_t)std::min<uint64_t>((n + kPolGradRows - 1u) / kPolGradRows, kPolGradAcc);
    const size_t wave_blocks = (size_t)kPolGroupWave * P.wave_acc;
    P.slab_off = take(wave_blocks * P.slab_stride);
    P.stash_off = take(policy_grad_stash_floats((uint32_t)wave_blocks));
    P.floats = std::max(off, cpu_floats);
    return MBOTS_OK;
}

// the host path reads the segments: 0 <= lo <= hi <= n, pairwise disjoint
int segments_check_host(const int32_t *segments, uint32_t groups, uint64_t n, const char *what)
{
    std::vector<std::pair<int64_t, uint32_t>> by_lo;
    for (uint32_t e = 0; e < 4u * groups; ++e) {
        const int64_t lo = segments[2u * e], hi = segments[2u * e + 1u];
        if (lo < 0 || lo > hi || hi > (int64_t)n)
            return fail(MBOTS_E_INVALID, "the segment [" + std::to_string(lo) + ", " + std::to_string(hi) + ") of " +
                                             pair_name(e) + " is not inside the " + std::to_string(n) + " " + what);
        if (hi > lo) by_lo.emplace_back(lo, e);
    }
    std::sort(by_lo.begin(), by_lo.end());
    for (size_t i = 1; i < by_lo.size(); ++i) {
        const uint32_t a = by_lo[i - 1].second, b = by_lo[i].second;
        if (segments[2u * a + 1u] > segments[2u * b])
            return fail(MBOTS_E_INVALID, "the segments of " + pair_name(a) + " and " + pair_name(b) + " overlap");
    }
    return MBOTS_OK;
}

int groups_check(const mbots_policy_net *nets, uint32_t groups, const int32_t *segments, const float *obs,
                 const float *hidden, const int32_t *action, uint64_t n, void *ws, uint64_t ws_bytes, int32_t device,
                 GroupsPlan &P)
{
    if (int rc = groups_plan(nets, groups, n, P)) return rc;
    if (!segments) return fail(MBOTS_E_INVALID, "null segments");
    if (n && (!obs || !action)) return fail(MBOTS_E_INVALID, "null obs or action");
    if (n && P.memory_in && !hidden)
        return fail(MBOTS_E_INVALID, "a net with MBOTS_POLICY_MEMORY_IN needs the rows' hidden floats");
    if (!ws || ((uintptr_t)ws & 15u)) return fail(MBOTS_E_INVALID, "the workspace must be 16-byte aligned memory");
    if (ws_bytes < P.floats * sizeof(float))
        return fail(MBOTS_E_INVALID, "workspace of " + std::to_string(ws_bytes) + " bytes, " +
                                         std::to_string(P.floats * sizeof(float)) +
                                         " needed (mbots_policy_groups_workspace)");
    if (device >= 0) return MBOTS_OK;
    return segments_check_host(segments, groups, n, "rows");
}
}  // namespace

int mbots_policy_groups_workspace(const struct mbots_policy_net *nets, uint32_t groups, uint64_t n, uint64_t *bytes)
{
    if (!bytes) return fail(MBOTS_E_INVALID, "null argument");
    GroupsPlan P;
    if (int rc = groups_plan(nets, groups, n, P)) return rc;
    *bytes = P.floats * sizeof(float);
    return MBOTS_OK;
}

int mbots_policy_eval_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *segments,
                             const float *obs, const float *hidden, const int32_t *action, uint64_t n, float *logp,
                             float *value, float *entropy, void *workspace, uint64_t workspace_bytes, int32_t device,
                             void *stream)
{
    using namespace mbots;
    GroupsPlan P;
    if (int rc = groups_check(nets, groups, segments, obs, hidden, action, n, workspace, workspace_bytes, device, P))
        return rc;
    if (device < 0) {
        // rows of no segment, or of a pair without a net: +0
        for (float *o : {logp, value, entropy})
            if (o) std::fill(o, o + n, 0.0f);
        for (uint32_t e : P.present) {
            const uint64_t lo = (uint64_t)segments[2u * e], len = (uint64_t)segments[2u * e + 1u] - lo;
            if (!len) continue;
            if (int rc = mbots_policy_eval(&nets[e], obs + lo * kPolObs, hidden ? hidden + lo * kHidden : nullptr,
                                           action + lo, len, logp ? logp + lo : nullptr, value ? value + lo : nullptr,
                                           entropy ? entropy + lo : nullptr, workspace, workspace_bytes, -1, nullptr))
                return fail_pair(rc, e);
        }
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(device));
    float *ws = static_cast<float *>(workspace);
    const PolEvalIO io{obs, hidden, action, nullptr, nullptr, nullptr, logp, value, entropy, n};
    HIP_TRY(launch_policy_eval_groups(io, segments, P.spec.data(), 4u * groups, ws,
                                      reinterpret_cast<PolGroupEntry *>(ws + P.table_off),
                                      reinterpret_cast<PolUpload *>(ws + P.upload_off), as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_grad_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *segments,
                             const float *obs, const float *hidden, const int32_t *action, uint64_t n,
                             const float *g_logp, const float *g_value, const float *g_entropy,
                             const struct mbots_policy_grads *out, void *workspace, uint64_t workspace_bytes,
                             int32_t device, void *stream)
{
    using namespace mbots;
    if (!out) return fail(MBOTS_E_INVALID, "null argument");
    GroupsPlan P;
    if (int rc = groups_check(nets, groups, segments, obs, hidden, action, n, workspace, workspace_bytes, device, P))
        return rc;
    if (device < 0) {
        for (uint32_t e : P.present) {
            const uint64_t lo = (uint64_t)segments[2u * e], len = (uint64_t)segments[2u * e + 1u] - lo;
            if (int rc = mbots_policy_grad(&nets[e], obs + lo * kPolObs, hidden ? hidden + lo * kHidden : nullptr,
                                           action + lo, len, g_logp ? g_logp + lo : nullptr,
                                           g_value ? g_value + lo : nullptr, g_entropy ? g_entropy + lo : nullptr,
                                           &out[e], workspace, workspace_bytes, -1, nullptr))
                return fail_pair(rc, e);
        }
        return MBOTS_OK;
    }
    // the present segments in waves, each with the pointers its reduce writes
    std::vector<PolGroupWave> waves((P.present.size() + kPolGroupWave - 1u) / kPolGroupWave);
    std::vector<PolGroupGrads> grads(waves.size());
    for (size_t i = 0; i < P.present.size(); ++i) {
        const uint32_t e = P.present[i], c = (uint32_t)(i % kPolGroupWave);
        PolGroupWave &W = waves[i / kPolGroupWave];
        PolGroupGrads &O = grads[i / kPolGroupWave];
        if (c == 0) W = PolGroupWave{}, O = PolGroupGrads{};
        W.seg[c] = e;
        W.n = c + 1u;
        for (uint32_t l = 0; l < P.spec[e].n_trunk; ++l)
            O.w[c][l] = out[e].trunk[l].weight, O.b[c][l] = out[e].trunk[l].bias;
        for (int k = 0; k < 2; ++k) {
            O.w[c][kPolMaxTrunk + k] = out[e].actor[k].weight, O.b[c][kPolMaxTrunk + k] = out[e].actor[k].bias;
            O.w[c][kPolMaxTrunk + 2 + k] = out[e].critic[k].weight, O.b[c][kPolMaxTrunk + 2 + k] = out[e].critic[k].bias;
        }
    }
    HIP_TRY(hipSetDevice(device));
    float *ws = static_cast<float *>(workspace);
    const PolEvalIO io{obs, hidden, action, g_logp, g_value, g_entropy, nullptr, nullptr, nullptr, n};
    HIP_TRY(launch_policy_grad_groups(io, segments, P.spec.data(), 4u * groups, waves.data(), grads.data(),
                                      (uint32_t)waves.size(), ws, reinterpret_cast<PolGroupEntry *>(ws + P.table_off),
                                      reinterpret_cast<PolUpload *>(ws + P.upload_off), ws + P.slab_off, P.slab_stride,
                                      ws + P.stash_off, P.wave_acc, as_stream(stream)));
    return MBOTS_OK;
}

// ---- the update on the device (include/mbots.h "The update on the device") ----
static_assert(sizeof(mbots_policy_adam_tensor) == sizeof(mbots::AdamTensor) &&
                  offsetof(mbots_policy_adam_tensor, group) == offsetof(mbots::AdamTensor, group) &&
                  sizeof(mbots_policy_adam_state) == sizeof(mbots::AdamState),
              "mbots.h's Adam structs are the kernels'");

namespace {
int adam_check(const mbots_policy_adam_tensor *tensors, uint64_t count, const mbots_policy_adam_state *state,
               uint32_t groups)
{
    if ((!tensors && count) || !state) return fail(MBOTS_E_INVALID, "null argument");
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    for (uint64_t i = 0; i < count; ++i) {
        const mbots_policy_adam_tensor &T = tensors[i];
        if (T.n == 0) continue;
        const uintptr_t bits = (uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.m | (uintptr_t)T.v;
        const char *bad = !T.param || !T.grad || !T.m || !T.v ? "has a null pointer"
                          : (bits & 3u)                       ? "is not 4-byte aligned"
                          : T.group >= groups                 ? "names a group past `groups`"
                          : T.n > (1ull << 31)                ? "has more than 2^31 elements"
                                                              : nullptr;
        if (bad) return fail(MBOTS_E_INVALID, "Adam tensor " + std::to_string(i) + " " + bad);
    }
    return MBOTS_OK;
}
}  // namespace

int mbots_policy_group_rows(const int32_t *segments, uint32_t groups, int64_t *rows, int32_t device, void *stream)
{
    if (!segments || !rows) return fail(MBOTS_E_INVALID, "null argument");
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    if (device < 0) {
        for (uint32_t e = 0; e < 4u * groups; ++e)
            if (segments[2u * e] < 0 || segments[2u * e] > segments[2u * e + 1u])
                return fail(MBOTS_E_INVALID, "the segment [" + std::to_string(segments[2u * e]) + ", " +
                                                 std::to_string(segments[2u * e + 1u]) + ") of " + pair_name(e) +
                                                 " is no row range");
        for (uint32_t e = 0; e < 4u * groups; ++e) rows[e / 4u] += (int64_t)segments[2u * e + 1u] - segments[2u * e];
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(mbots::launch_policy_group_rows(segments, groups, rows, as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_a2c_loss(const float *logp, const float *value, const float *entropy, const float *adv,
                          const float *ret, const int32_t *end, uint64_t n, const int32_t *segments, uint32_t groups,
                          const int64_t *rows, float value_coef, float entropy_coef, float *g_logp, float *g_value,
                          float *g_entropy, double *loss, int32_t device, void *stream)
{
    using namespace mbots;
    if (!segments || !rows) return fail(MBOTS_E_INVALID, "null segments or rows");
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    if (n && (!logp || !value || !entropy || !adv || !ret)) return fail(MBOTS_E_INVALID, "null argument");
    if (n > (uint64_t)INT32_MAX) return fail(MBOTS_E_INVALID, "more rows than a segment can name");
    const PolLossIO io{logp,   value,   entropy,   adv,  ret, end,        segments,    rows,
                       g_logp, g_value, g_entropy, loss, n,   value_coef, entropy_coef};
    if (device >= 0) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_a2c_loss(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = segments_check_host(segments, groups, n, "rows")) return rc;
    for (float *o : {g_logp, g_value, g_entropy})
        if (o) std::fill(o, o + n, 0.0f);
    for (uint32_t g = 0; g < groups; ++g) {
        const float scale = pol_loss_scale(rows[g]);
        double group_sum = 0.0;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint64_t lo = (uint64_t)segments[2u * (4u * g + s)];
            const uint64_t len = (uint64_t)segments[2u * (4u * g + s) + 1u] - lo;
            double acc[kLossAcc] = {};
            for (uint64_t i = 0; i < len; ++i) {
                const uint64_t r = lo + i;
                const float w = (end && end[r] == kTrajEndReset ? 0.0f : 1.0f) * scale;
                float gl, gv, ge;
                const float per_row = pol_loss_row(logp[r], value[r], entropy[r], adv[r], ret[r], w, value_coef,
                                                   entropy_coef, gl, gv, ge);
                if (g_logp) g_logp[r] = gl;
                if (g_value) g_value[r] = gv;
                if (g_entropy) g_entropy[r] = ge;
                acc[i % kLossAcc] += (double)per_row;
            }
            double q = 0.0;
            for (uint32_t k = 0; k < kLossAcc; ++k) q += acc[k];
            group_sum += q;
        }
        if (loss) loss[g] += group_sum;
    }
    return MBOTS_OK;
}

int mbots_policy_adam(const struct mbots_policy_adam_tensor *tensors, uint64_t count,
                      struct mbots_policy_adam_state *state, uint32_t groups, const int64_t *rows, float lr,
                      float beta1, float beta2, float eps, int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = adam_check(tensors, count, state, groups)) return rc;
    const AdamCoef C{lr, beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
    if (device >= 0) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_adam(reinterpret_cast<const AdamTensor *>(tensors), count,
                                   reinterpret_cast<AdamState *>(state), groups, rows, C, as_stream(stream)));
        return MBOTS_OK;
    }
    for (uint64_t i = 0; i < count; ++i) {
        const mbots_policy_adam_tensor &T = tensors[i];
        if (T.n == 0 || (rows && rows[T.group] == 0)) continue;
        const float c1 = 1.0f - state[T.group].b1t * beta1, c2 = 1.0f - state[T.group].b2t * beta2;
        for (uint64_t k = 0; k < T.n; ++k) pol_adam(T.param[k], T.grad[k], T.m[k], T.v[k], C, c1, c2);
    }
    for (uint32_t g = 0; g < groups; ++g) {
        if (rows && rows[g] == 0) continue;
        state[g].t += 1u;
        state[g].b1t = state[g].b1t * beta1;
        state[g].b2t = state[g].b2t * beta2;
    }
    return MBOTS_OK;
}

// ---- evaluate_sequences (include/mbots.h "Training the memory head") ----
namespace {
int seq_check(const mbots_policy_net *net, const float *obs, const int32_t *action, const int32_t *length,
              const float *hidden0, uint32_t L, uint64_t B, void *ws, uint64_t ws_bytes, int32_t device, EvalPlan &P)
{
    if (!net) return fail(MBOTS_E_INVALID, "null argument");
    if (int rc = eval_plan(net, B, device < 0, static_cast<float *>(ws), P, EvalMode{true, L})) return rc;
    if (B && L && (!obs || !action)) return fail(MBOTS_E_INVALID, "null obs or action");
    if (B && (!length || !hidden0)) return fail(MBOTS_E_INVALID, "null length or hidden0");
    if (!ws || ((uintptr_t)ws & 15u)) return fail(MBOTS_E_INVALID, "the workspace must be 16-byte aligned memory");
    if (ws_bytes < P.floats * sizeof(float))
        return fail(MBOTS_E_INVALID, "workspace of " + std::to_string(ws_bytes) + " bytes, " +
                                         std::to_string(P.floats * sizeof(float)) + " needed (mbots_policy_seq_workspace)");
    if (device < 0)
        for (uint64_t b = 0; b < B; ++b) {
            if (length[b] < 0 || (uint32_t)length[b] > L)
                return fail(MBOTS_E_INVALID, "length " + std::to_string(length[b]) + " of sequence " + std::to_string(b) +
                                                 " is outside [0, " + std::to_string(L) + "]");
            for (int32_t k = 0; k < length[b]; ++k) {
                const int32_t a = action[(uint64_t)k * B + b];
                if (a < 0 || a >= mbots::kPolActions)
                    return fail(MBOTS_E_INVALID, "action " + std::to_string(a) + " of step " + std::to_string(k) +
                                                     " of sequence " + std::to_string(b) + " is outside 0..5");
            }
        }
    return MBOTS_OK;
}
}  // namespace

int mbots_policy_seq_workspace(const struct mbots_policy_net *net, uint32_t L, uint64_t B, uint64_t *bytes)
{
    if (!net || !bytes) return fail(MBOTS_E_INVALID, "null argument");
    EvalPlan P;
    if (int rc = eval_plan(net, B, false, nullptr, P, EvalMode{true, L})) return rc;
    *bytes = P.floats * sizeof(float);
    return MBOTS_OK;
}

int mbots_policy_seq_eval(const struct mbots_policy_net *net, const float *obs, const int32_t *action,
                          const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, float *logp,
                          float *value, float *entropy, float *hidden, void *workspace, uint64_t workspace_bytes,
                          int32_t device, void *stream)
{
    EvalPlan P;
    if (int rc = seq_check(net, obs, action, length, hidden0, L, B, workspace, workspace_bytes, device, P)) return rc;
    const mbots::PolSeqIO io{obs, hidden0, action, length, nullptr, nullptr, nullptr, logp, value, entropy, hidden, L, B};
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = eval_upload(P, false, device, as_stream(stream))) return rc;
    if (device < 0) {
        mbots::cpu::policy_seq_eval(P.net, io);
        return MBOTS_OK;
    }
    HIP_TRY(mbots::launch_policy_seq_eval(io, P.net, as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_seq_grad(const struct mbots_policy_net *net, const float *obs, const int32_t *action,
                          const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, const float *g_logp,
                          const float *g_value, const float *g_entropy, const struct mbots_policy_grads *out,
                          void *workspace, uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (!out) return fail(MBOTS_E_INVALID, "null argument");
    EvalPlan P;
    if (int rc = seq_check(net, obs, action, length, hidden0, L, B, workspace, workspace_bytes, device, P)) return rc;
    for (uint32_t l = 0; l < P.net.n_trunk; ++l) P.out.w[l] = out->trunk[l].weight, P.out.b[l] = out->trunk[l].bias;
    for (int i = 0; i < 2; ++i) {
        P.out.w[kPolMaxTrunk + i] = out->actor[i].weight;
        P.out.b[kPolMaxTrunk + i] = out->actor[i].bias;
        P.out.w[kPolMaxTrunk + 2 + i] = out->critic[i].weight;
        P.out.b[kPolMaxTrunk + 2 + i] = out->critic[i].bias;
    }
    P.out.w[kPolGradLayers] = out->memory.weight;
    P.out.b[kPolGradLayers] = out->memory.bias;
    if (P.net.gated) {
        P.out.w[kPolSeqLayers] = out->gate.weight;
        P.out.b[kPolSeqLayers] = out->gate.bias;
    }
    const PolSeqIO io{obs, hidden0, action, length, g_logp, g_value, g_entropy, nullptr, nullptr, nullptr, nullptr, L, B};
    float *ws = static_cast<float *>(workspace);
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = eval_upload(P, true, device, as_stream(stream))) return rc;
    if (device < 0) {
        cpu::policy_seq_grad(P.net, io, P.slabs, ws + P.h_off, P.out);
        return MBOTS_OK;
    }
    HIP_TRY(launch_policy_seq_grad(io, P.net, P.back, P.slabs, ws + P.stash_off, ws + P.h_off, P.out, as_stream(stream)));
    return MBOTS_OK;
}

// ---- grouped evaluate_sequences (include/mbots.h "Every group's recurrent nets
// in one call") ----
namespace {
// where a grouped sequence call's pieces lie in the caller's workspace (floats):
// GroupsPlan's, and one wave's h stores
struct SeqGroupsPlan {
    std::vector<mbots::PolSeqGroupSpec> spec;   // [4 groups]; n_trunk == 0: no net
    std::vector<uint32_t> present;
    size_t table_off = 0, upload_off = 0, slab_off = 0, stash_off = 0, h_off = 0, floats = 0;
    uint64_t slab_stride = 0;
    uint32_t wave_acc = 0;
};

int seq_groups_plan(const mbots_policy_net *nets, uint32_t groups, uint32_t L, uint64_t B, SeqGroupsPlan &P)
{
    using namespace mbots;
    if (!nets) return fail(MBOTS_E_INVALID, "null nets");
    if (groups < 1 || groups > kPolMaxGroups)
        return fail(MBOTS_E_INVALID, "1.." + std::to_string(kPolMaxGroups) + " groups, not " + std::to_string(groups));
    if (B > 0x7FFFFFFFull) return fail(MBOTS_E_INVALID, "order addresses columns as int32: at most 2^31 - 1 sequences");
    const uint32_t nseg = 4u * groups;
    P.spec.assign(nseg, PolSeqGroupSpec{});
    size_t off = 0, cpu_floats = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 63u) & ~size_t(63);
        return at;
    };
    P.table_off = take((size_t)nseg * sizeof(PolGroupEntry) / sizeof(float));
    P.upload_off = take((size_t)nseg * kPolSeqGroupUploads * sizeof(PolUpload) / sizeof(float));
    for (uint32_t e = 0; e < nseg; ++e) {
        const mbots_policy_net &src = nets[e];
        if (src.n_trunk == 0) continue;
        PolNet d;
        if (int rc = policy_describe(&src, d)) return fail_pair(rc, e);
        if (!(d.has_memory && (d.flags & kPolMemoryIn)))
            return fail(MBOTS_E_INVALID, pair_name(e) + ": sequences are evaluated by a net with a memory head and "
                                                        "MBOTS_POLICY_MEMORY_IN (mbots_policy_eval_groups evaluates "
                                                        "the nets without them)");
        PolGroupSpec &s = P.spec[e].s;
        s.w_off = off;
        s.n_trunk = d.n_trunk;
        s.H = d.H;
        s.flags = d.flags;
        for (uint32_t l = 0; l < d.n_trunk; ++l) {
            s.act |= d.trunk[l].act << (8u * l);
            s.w[l] = src.trunk[l].weight, s.b[l] = src.trunk[l].bias;
        }
        for (int i = 0; i < 2; ++i) {
            s.w[kPolMaxTrunk + i] = src.actor[i].weight, s.b[kPolMaxTrunk + i] = src.actor[i].bias;
            s.w[kPolMaxTrunk + 2 + i] = src.critic[i].weight, s.b[kPolMaxTrunk + 2 + i] = src.critic[i].bias;
        }
        P.spec[e].mw = src.memory.weight;
        P.spec[e].mb = src.memory.bias;
        if (d.gated) {
            P.spec[e].gw = src.gate.weight;
            P.spec[e].gb = src.gate.bias;
        }
        PolGroupEntry E;
        off += pol_group_entry(s, nullptr, E, nullptr, kPolSeqGroupUploads, true);
        P.slab_stride = std::max<uint64_t>(P.slab_stride, E.slab_floats);
        P.present.push_back(e);
        // (the host path runs evaluate_sequences' own plan, one net at a time, in the same memory)
        EvalPlan one;
        if (int rc = eval_plan(&src, B, true, nullptr, one, EvalMode{true, L})) return fail_pair(rc, e);
        cpu_floats = std::max(cpu_floats, one.floats);
    }
    P.wave_acc = (uint32_t)std::min<uint64_t>((B + kPolGradRows - 1u) / kPolGradRows, kPolGradAcc);
    const size_t wave_blocks = (size_t)kPolGroupWave * P.wave_acc;
    P.slab_off = take(wave_blocks * P.slab_stride);
    P.stash_off = take(policy_grad_stash_floats((uint32_t)wave_blocks));
    P.h_off = take(pol_seq_h_floats((uint32_t)wave_blocks, L));
    P.floats = std::max(off, cpu_floats);
    return MBOTS_OK;
}

int seq_groups_check(const mbots_policy_net *nets, uint32_t groups, const int32_t *order, const int32_t *segments,
                     const float *obs, const int32_t *action, const int32_t *length, const float *hidden0, uint32_t L,
                     uint64_t B, void *ws, uint64_t ws_bytes, int32_t device, SeqGroupsPlan &P)
{
    if (int rc = seq_groups_plan(nets, groups, L, B, P)) return rc;
    if (!segments) return fail(MBOTS_E_INVALID, "null segments");
    if (B && !order) return fail(MBOTS_E_INVALID, "null order");
    if (B && L && (!obs || !action)) return fail(MBOTS_E_INVALID, "null obs or action");
    if (B && (!length || !hidden0)) return fail(MBOTS_E_INVALID, "null length or hidden0");
    if (!ws || ((uintptr_t)ws & 15u)) return fail(MBOTS_E_INVALID, "the workspace must be 16-byte aligned memory");
    if (ws_bytes < P.floats * sizeof(float))
        return fail(MBOTS_E_INVALID, "workspace of " + std::to_string(ws_bytes) + " bytes, " +
                                         std::to_string(P.floats * sizeof(float)) +
                                         " needed (mbots_policy_seq_groups_workspace)");
    if (device >= 0) return MBOTS_OK;
    // the host path reads everything: the segments, then every evaluated column
    if (int rc = segments_check_host(segments, groups, B, "positions of order")) return rc;
    std::vector<uint8_t> seen(B, 0);
    for (uint32_t e : P.present)
        for (int64_t p = segments[2u * e]; p < segments[2u * e + 1u]; ++p) {
            const int64_t b = order[p];
            const std::string at = pair_name(e) + ": order[" + std::to_string(p) + "] = " + std::to_string(b);
            if (b < 0 || b >= (int64_t)B)
                return fail(MBOTS_E_INVALID, at + " is outside the " + std::to_string(B) + " sequences");
            if (seen[b]) return fail(MBOTS_E_INVALID, at + " names a sequence a second time");
            seen[b] = 1;
            if (length[b] < 0 || (uint32_t)length[b] > L)
                return fail(MBOTS_E_INVALID, pair_name(e) + ": length " + std::to_string(length[b]) + " of sequence " +
                                                 std::to_string(b) + " is outside [0, " + std::to_string(L) + "]");
            for (int32_t k = 0; k < length[b]; ++k) {
                const int32_t a = action[(uint64_t)k * B + b];
                if (a < 0 || a >= mbots::kPolActions)
                    return fail(MBOTS_E_INVALID, pair_name(e) + ": action " + std::to_string(a) + " of step " +
                                                     std::to_string(k) + " of sequence " + std::to_string(b) +
                                                     " is outside 0..5");
            }
        }
    return MBOTS_OK;
}

// the caller's gradient pointers of net `src`'s layers, in PolGradOut's slots
void seq_grad_slots(const mbots_policy_grads &out, uint32_t n_trunk, bool gated, float **w, float **b)
{
    using namespace mbots;
    for (int i = 0; i < kPolGateLayers; ++i) w[i] = b[i] = nullptr;
    if (gated) w[kPolSeqLayers] = out.gate.weight, b[kPolSeqLayers] = out.gate.bias;
    for (uint32_t l = 0; l < n_trunk; ++l) w[l] = out.trunk[l].weight, b[l] = out.trunk[l].bias;
    for (int i = 0; i < 2; ++i) {
        w[kPolMaxTrunk + i] = out.actor[i].weight, b[kPolMaxTrunk + i] = out.actor[i].bias;
        w[kPolMaxTrunk + 2 + i] = out.critic[i].weight, b[kPolMaxTrunk + 2 + i] = out.critic[i].bias;
    }
    w[kPolGradLayers] = out.memory.weight, b[kPolGradLayers] = out.memory.bias;
}
}  // namespace

int mbots_policy_seq_order(const int32_t *net_id, uint64_t B, uint32_t groups, int32_t *order, int32_t *segments,
                           void *workspace, uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (groups < 1 || groups > kPolMaxGroups)
        return fail(MBOTS_E_INVALID, "1.." + std::to_string(kPolMaxGroups) + " groups, not " + std::to_string(groups));
    if (B > 0x7FFFFFFFull) return fail(MBOTS_E_INVALID, "order addresses columns as int32: at most 2^31 - 1 sequences");
    if (!segments || (B && (!net_id || !order))) return fail(MBOTS_E_INVALID, "null argument");
    const uint32_t nkeys = 4u * groups;
    if (device < 0) {
        // the stable counting sort on the host: count, scan, scatter in column order
        std::vector<uint32_t> at(nkeys + 1u, 0u);
        for (uint64_t b = 0; b < B; ++b)
            if (pol_seq_key(net_id[b], nkeys)) ++at[(uint32_t)net_id[b] + 1u];
        for (uint32_t k = 0; k < nkeys; ++k) {
            at[k + 1u] += at[k];
            segments[2u * k] = (int32_t)at[k];
            segments[2u * k + 1u] = (int32_t)at[k + 1u];
        }
        for (uint64_t p = at[nkeys]; p < B; ++p) order[p] = -1;
        for (uint64_t b = 0; b < B; ++b)
            if (pol_seq_key(net_id[b], nkeys)) order[at[(uint32_t)net_id[b]]++] = (int32_t)b;
        return MBOTS_OK;
    }
    const uint64_t need = policy_seq_order_workspace(B);
    if (!workspace || ((uintptr_t)workspace & 3u) || workspace_bytes < need)
        return fail(MBOTS_E_INVALID, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) +
                                         " needed (MBOTS_POLICY_SEQ_ORDER_WORKSPACE(B))");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_seq_order(net_id, B, nkeys, order, segments, static_cast<uint32_t *>(workspace),
                                    as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_seq_groups_workspace(const struct mbots_policy_net *nets, uint32_t groups, uint32_t L, uint64_t B,
                                      uint64_t *bytes)
{
    if (!bytes) return fail(MBOTS_E_INVALID, "null argument");
    SeqGroupsPlan P;
    if (int rc = seq_groups_plan(nets, groups, L, B, P)) return rc;
    *bytes = P.floats * sizeof(float);
    return MBOTS_OK;
}

int mbots_policy_seq_eval_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *order,
                                 const int32_t *segments, const float *obs, const int32_t *action,
                                 const int32_t *length, const float *hidden0, uint32_t L, uint64_t B, float *logp,
                                 float *value, float *entropy, float *hidden, void *workspace, uint64_t workspace_bytes,
                                 int32_t device, void *stream)
{
    using namespace mbots;
    SeqGroupsPlan P;
    if (int rc = seq_groups_check(nets, groups, order, segments, obs, action, length, hidden0, L, B, workspace,
                                  workspace_bytes, device, P))
        return rc;
    const PolSeqIO io{obs, hidden0, action, length, nullptr, nullptr, nullptr, logp, value, entropy, hidden, L, B};
    float *ws = static_cast<float *>(workspace);
    if (device < 0) {
        // columns of no segment, or of a pair without a net: +0
        for (float *o : {logp, value, entropy})
            if (o) std::fill(o, o + (uint64_t)L * B, 0.0f);
        if (hidden) std::fill(hidden, hidden + (uint64_t)L * B * kHidden, 0.0f);
        for (uint32_t e : P.present) {
            const uint64_t lo = (uint64_t)segments[2u * e], len = (uint64_t)segments[2u * e + 1u] - lo;
            if (!len) continue;
            EvalPlan one;
            if (int rc = eval_plan(&nets[e], len, true, ws, one, EvalMode{true, L})) return fail_pair(rc, e);
            if (int rc = eval_upload(one, false, -1, nullptr)) return fail_pair(rc, e);
            cpu::policy_seq_eval(one.net, io, PolSeqCols{order + lo, len});
        }
        return MBOTS_OK;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_seq_eval_groups(io, order, segments, P.spec.data(), 4u * groups, ws,
                                          reinterpret_cast<PolGroupEntry *>(ws + P.table_off),
                                          reinterpret_cast<PolUpload *>(ws + P.upload_off), as_stream(stream)));
    return MBOTS_OK;
}

int mbots_policy_seq_grad_groups(const struct mbots_policy_net *nets, uint32_t groups, const int32_t *order,
                                 const int32_t *segments, const float *obs, const int32_t *action,
                                 const int32_t *length, const float *hidden0, uint32_t L, uint64_t B,
                                 const float *g_logp, const float *g_value, const float *g_entropy,
                                 const struct mbots_policy_grads *out, void *workspace, uint64_t workspace_bytes,
                                 int32_t device, void *stream)
{
    using namespace mbots;
    if (!out) return fail(MBOTS_E_INVALID, "null argument");
    SeqGroupsPlan P;
    if (int rc = seq_groups_check(nets, groups, order, segments, obs, action, length, hidden0, L, B, workspace,
                                  workspace_bytes, device, P))
        return rc;
    const PolSeqIO io{obs, hidden0, action, length, g_logp, g_value, g_entropy, nullptr, nullptr, nullptr, nullptr, L, B};
    float *ws = static_cast<float *>(workspace);
    if (device < 0) {
        for (uint32_t e : P.present) {
            const uint64_t lo = (uint64_t)segments[2u * e], len = (uint64_t)segments[2u * e + 1u] - lo;
            EvalPlan one;
            if (int rc = eval_plan(&nets[e], len, true, ws, one, EvalMode{true, L})) return fail_pair(rc, e);
            seq_grad_slots(out[e], one.net.n_trunk, one.net.gated != 0u, one.out.w, one.out.b);
            if (int rc = eval_upload(one, true, -1, nullptr)) return fail_pair(rc, e);
            cpu::policy_seq_grad(one.net, io, one.slabs, ws + one.h_off, one.out, PolSeqCols{order + lo, len});
        }
        return MBOTS_OK;
    }
    // the present segments in waves, each with the pointers its reduce writes
    std::vector<PolGroupWave> waves((P.present.size() + kPolGroupWave - 1u) / kPolGroupWave);
    std::vector<PolSeqGroupGrads> grads(waves.size());
    for (size_t i = 0; i < P.present.size(); ++i) {
        const uint32_t e = P.present[i], c = (uint32_t)(i % kPolGroupWave);
        PolGroupWave &W = waves[i / kPolGroupWave];
        PolSeqGroupGrads &O = grads[i / kPolGroupWave];
        if (c == 0) W = PolGroupWave{}, O = PolSeqGroupGrads{};
        W.seg[c] = e;
        W.n = c + 1u;
        seq_grad_slots(out[e], P.spec[e].s.n_trunk, (P.spec[e].s.flags & kPolGate) != 0u, O.w[c], O.b[c]);
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_seq_grad_groups(io, order, segments, P.spec.data(), 4u * groups, waves.data(), grads.data(),
                                          (uint32_t)waves.size(), ws,
                                          reinterpret_cast<PolGroupEntry *>(ws + P.table_off),
                                          reinterpret_cast<PolUpload *>(ws + P.upload_off), ws + P.slab_off,
                                          P.slab_stride, ws + P.stash_off, ws + P.h_off, P.wave_acc, as_stream(stream)));
    return MBOTS_OK;
}

// ---- the recurrent update on the device (include/mbots.h "The update on the
// device": the sequence batches, clipping and weight decay) ----
namespace {
// the host path of the sequence loss reads everything first: the segments, then
// every column they name (L == 0: the lengths are not bounded)
int seq_loss_check_host(const int32_t *order, const int32_t *segments, uint32_t groups, const int32_t *len, uint32_t L,
                        uint64_t B)
{
    if (int rc = segments_check_host(segments, groups, B, "positions of order")) return rc;
    std::vector<uint8_t> seen(B, 0);
    for (uint32_t e = 0; e < 4u * groups; ++e)
        for (int64_t p = segments[2u * e]; p < segments[2u * e + 1u]; ++p) {
            const int64_t b = order[p];
            const std::string at = pair_name(e) + ": order[" + std::to_string(p) + "] = " + std::to_string(b);
            if (b < 0 || b >= (int64_t)B)
                return fail(MBOTS_E_INVALID, at + " is outside the " + std::to_string(B) + " sequences");
            if (seen[b]) return fail(MBOTS_E_INVALID, at + " names a sequence a second time");
            seen[b] = 1;
            if (L && (len[b] < 0 || (uint32_t)len[b] > L))
                return fail(MBOTS_E_INVALID, pair_name(e) + ": length " + std::to_string(len[b]) + " of sequence " +
                                                 std::to_string(b) + " is outside [0, " + std::to_string(L) + "]");
        }
    return MBOTS_OK;
}

int seq_loss_args(uint32_t groups, uint64_t B, const int32_t *len, const int32_t *t0, const int32_t *end,
                  const int32_t *order, const int32_t *segments, const int64_t *rows)
{
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    if (B > 0x7FFFFFFFull) return fail(MBOTS_E_INVALID, "order addresses columns as int32: at most 2^31 - 1 sequences");
    if (!segments || !rows) return fail(MBOTS_E_INVALID, "null segments or rows");
    if (B && (!len || !t0 || !end || !order)) return fail(MBOTS_E_INVALID, "null len, t0, end or order");
    return MBOTS_OK;
}

// a chunk's squared norm on the host: policy_adam_sq_kernel's accumulators and tree
double adam_chunk_sq(const float *g, uint32_t cnt)
{
    using namespace mbots;
    double a[kAdamChunk / 4u];
    for (uint32_t j = 0; j < kAdamChunk / 4u; ++j) {
        float x[4];
        for (uint32_t k = 0; k < 4u; ++k) x[k] = 4u * j + k < cnt ? g[4u * j + k] : 0.0f;
        a[j] = pol_sq4(x[0], x[1], x[2], x[3]);
    }
    for (uint32_t h = kAdamChunk / 8u; h > 0u; h >>= 1)
        for (uint32_t i = 0; i < h; ++i) a[i] = a[i] + a[i + h];
    return a[0];
}
}  // namespace

int mbots_policy_seq_group_rows(const int32_t *len, const int32_t *t0, const int32_t *end, uint64_t B,
                                const int32_t *order, const int32_t *segments, uint32_t groups, int32_t last_table,
                                int64_t *rows, int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = seq_loss_args(groups, B, len, t0, end, order, segments, rows)) return rc;
    if (device >= 0) {
        PolSeqLossIO io{};
        io.len = len, io.t0 = t0, io.end = end, io.order = order, io.segments = segments;
        io.B = B, io.last_table = last_table;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_seq_group_rows(io, groups, rows, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = seq_loss_check_host(order, segments, groups, len, 0, B)) return rc;
    for (uint32_t e = 0; e < 4u * groups; ++e)
        for (int64_t p = segments[2u * e]; p < segments[2u * e + 1u]; ++p) {
            const int32_t b = order[p];
            rows[e / 4u] += pol_seq_kept(len[b], t0[b], end[b], last_table);
        }
    return MBOTS_OK;
}

int mbots_policy_seq_a2c_loss(const float *logp, const float *value, const float *entropy, const float *adv,
                              const float *ret, const int32_t *len, const int32_t *t0, const int32_t *end, uint32_t L,
                              uint64_t B, const int32_t *order, const int32_t *segments, uint32_t groups,
                              int32_t last_table, const int64_t *rows, float value_coef, float entropy_coef,
                              float *g_logp, float *g_value, float *g_entropy, double *loss, int32_t device,
                              void *stream)
{
    using namespace mbots;
    if (int rc = seq_loss_args(groups, B, len, t0, end, order, segments, rows)) return rc;
    if (L && B && (!logp || !value || !entropy || !adv || !ret)) return fail(MBOTS_E_INVALID, "null argument");
    if (L > (uint32_t)INT32_MAX) return fail(MBOTS_E_INVALID, "L is no int32 length");
    const PolSeqLossIO io{logp,   value,   entropy,   adv,  ret, len, t0, end,        order,      segments,    rows,
                          g_logp, g_value, g_entropy, loss, L,   B,   last_table, value_coef, entropy_coef};
    if (device >= 0) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_seq_a2c_loss(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = seq_loss_check_host(order, segments, groups, len, L ? L : 1u, B)) return rc;
    for (float *o : {g_logp, g_value, g_entropy})
        if (o) std::fill(o, o + (uint64_t)L * B, 0.0f);
    for (uint32_t g = 0; g < groups; ++g) {
        if (rows[g] == 0) continue;   // the +0 stay, the loss is not touched
        const float w = pol_loss_scale(rows[g]);
        double group_sum = 0.0;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint64_t lo = (uint64_t)segments[2u * (4u * g + s)];
            const uint64_t n = (uint64_t)segments[2u * (4u * g + s) + 1u] - lo;
            double acc[kLossAcc] = {};
            for (uint64_t i = 0; i < n; ++i) {
                const int32_t b = order[lo + i];
                const int32_t nk = std::min(pol_seq_kept(len[b], t0[b], end[b], last_table), (int32_t)L);
                for (int32_t k = 0; k < nk; ++k) {
                    const uint64_t r = (uint64_t)k * B + (uint32_t)b;
                    float gl, gv, ge;
                    const float per_row = pol_loss_row(logp[r], value[r], entropy[r], adv[r], ret[r], w, value_coef,
                                                       entropy_coef, gl, gv, ge);
                    if (g_logp) g_logp[r] = gl;
                    if (g_value) g_value[r] = gv;
                    if (g_entropy) g_entropy[r] = ge;
                    acc[i % kLossAcc] += (double)per_row;
                }
            }
            double q = 0.0;
            for (uint32_t k = 0; k < kLossAcc; ++k) q += acc[k];
            group_sum += q;
        }
        if (loss) loss[g] += group_sum;
    }
    return MBOTS_OK;
}

int mbots_policy_adam_clip_workspace(const struct mbots_policy_adam_tensor *tensors, uint64_t count, uint32_t groups,
                                     uint64_t *bytes)
{
    using namespace mbots;
    if ((!tensors && count) || !bytes) return fail(MBOTS_E_INVALID, "null argument");
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    uint64_t chunks, present;
    policy_adam_clip_counts(reinterpret_cast<const AdamTensor *>(tensors), count, chunks, present);
    *bytes = pol_adam_clip_bytes(chunks, present, groups);
    return MBOTS_OK;
}

int mbots_policy_adam_clip(const struct mbots_policy_adam_tensor *tensors, uint64_t count,
                           struct mbots_policy_adam_state *state, uint32_t groups, const int64_t *rows, float lr,
                           float beta1, float beta2, float eps, float weight_decay, float max_norm, float *grad_norm,
                           void *workspace, uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = adam_check(tensors, count, state, groups)) return rc;
    const AdamTensor *T = reinterpret_cast<const AdamTensor *>(tensors);
    uint64_t chunks, present;
    policy_adam_clip_counts(T, count, chunks, present);
    const uint64_t need = pol_adam_clip_bytes(chunks, present, groups);
    if (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < need)
        return fail(MBOTS_E_INVALID, "8-byte aligned workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                         std::to_string(need) + " needed (mbots_policy_adam_clip_workspace)");
    const AdamCoef C{lr, beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
    const AdamClipCoef K{lr * weight_decay, max_norm, max_norm > 0.0f && max_norm < INFINITY ? 1u : 0u,
                         weight_decay != 0.0f ? 1u : 0u};
    if (device >= 0) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_adam_clip(T, count, reinterpret_cast<AdamState *>(state), groups, rows, C, K, grad_norm,
                                        workspace, as_stream(stream)));
        return MBOTS_OK;
    }
    const AdamClipWs W = pol_adam_clip_ws(workspace, chunks, present, groups);
    for (uint32_t g = 0; g < groups; ++g) W.normsq[g] = 0.0;
    uint64_t c = 0, slot = 0;
    for (uint64_t i = 0; i < count; ++i) {
        if (T[i].n == 0) continue;
        double sum = 0.0;
        for (uint64_t base = 0; base < T[i].n; base += kAdamChunk) {
            W.q[c] = adam_chunk_sq(T[i].grad + base, (uint32_t)std::min<uint64_t>(kAdamChunk, T[i].n - base));
            sum += W.q[c++];
        }
        W.tsum[slot++] = sum;
        W.normsq[T[i].group] += sum;
    }
    for (uint32_t g = 0; g < groups; ++g) {
        float nrm;
        const bool finite = pol_clip_coef(W.normsq[g], K, nrm, W.coef[g]);
        W.live[g] = finite && (!rows || rows[g] != 0) ? 1u : 0u;
        if (grad_norm) grad_norm[g] = nrm;
    }
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t g = T[i].group;
        if (T[i].n == 0 || !W.live[g]) continue;
        const float c1 = 1.0f - state[g].b1t * beta1, c2 = 1.0f - state[g].b2t * beta2;
        for (uint64_t k = 0; k < T[i].n; ++k)
            pol_adam_clip(T[i].param[k], T[i].grad[k], T[i].m[k], T[i].v[k], C, K, W.coef[g], c1, c2);
    }
    for (uint32_t g = 0; g < groups; ++g) {
        if (!W.live[g]) continue;
        state[g].t += 1u;
        state[g].b1t = state[g].b1t * beta1;
        state[g].b2t = state[g].b2t * beta2;
    }
    return MBOTS_OK;
}

// ---- PPO on the device (include/mbots.h "PPO on the device") ----
namespace {
int ppo_groups_check(uint32_t groups)
{
    if (groups < 1u || groups > MBOTS_POLICY_MAX_GROUPS)
        return fail(MBOTS_E_INVALID, "groups must be 1.." + std::to_string(MBOTS_POLICY_MAX_GROUPS));
    return MBOTS_OK;
}

int ppo_workspace_check(const void *workspace, uint64_t workspace_bytes, uint64_t need)
{
    if (need && (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < need))
        return fail(MBOTS_E_INVALID, "8-byte aligned workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                         std::to_string(need) + " needed (mbots_policy_ppo_workspace)");
    return MBOTS_OK;
}

int ppo_coef(float clip, float value_clip, const float *old_value, float value_coef, float entropy_coef,
             mbots::PpoCoef &C)
{
    if (!(clip > 0.0f && clip < 1.0f)) return fail(MBOTS_E_INVALID, "clip must lie in (0, 1)");
    if (!(value_coef >= 0.0f)) return fail(MBOTS_E_INVALID, "value_coef must not be negative");
    C = mbots::PpoCoef{1.0f - clip, 1.0f + clip, value_clip, value_coef, entropy_coef,
                       value_clip > 0.0f && old_value ? 1u : 0u};
    return MBOTS_OK;
}

// The two-level order on the host: out[0 .. kSlots) += group g's sums, elem(s,
// position, acc) adding an element's shares to its accumulator.
extern "C++" template <uint32_t kSlots, class Elem>
void ppo_host_sum(const int32_t *segments, uint32_t g, uint32_t chunk, double *out, Elem &&elem)
{
    using namespace mbots;
    double group[kSlots] = {};
    std::vector<double> acc((size_t)kLossAcc * kSlots);
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint64_t lo = (uint64_t)segments[2u * (4u * g + s)];
        const uint64_t len = (uint64_t)segments[2u * (4u * g + s) + 1u] - lo;
        double seg[kSlots] = {};
        for (uint64_t first = 0; first < len; first += chunk) {
            std::fill(acc.begin(), acc.end(), 0.0);
            const uint64_t stop = std::min<uint64_t>(len, first + chunk);
            for (uint64_t i = first; i < stop; ++i) elem(lo + i, &acc[(i % kLossAcc) * kSlots]);
            for (uint32_t k = 0; k < kSlots; ++k) {
                double q = 0.0;
                for (uint32_t j = 0; j < kLossAcc; ++j) q += acc[(size_t)j * kSlots + k];
                seg[k] += q;
            }
        }
        for (uint32_t k = 0; k < kSlots; ++k) group[k] += seg[k];
    }
    for (uint32_t k = 0; k < kSlots; ++k) out[k] += group[k];
}
}  // namespace

int mbots_policy_ppo_workspace(uint64_t n, uint32_t groups, uint64_t *bytes)
{
    using namespace mbots;
    if (!bytes) return fail(MBOTS_E_INVALID, "null argument");
    if (int rc = ppo_groups_check(groups)) return rc;
    *bytes = pol_ppo_bytes(std::max(pol_ppo_chunks(n, kPpoChunk), pol_ppo_chunks(n, kPpoSeqChunk)), groups);
    return MBOTS_OK;
}

int mbots_policy_adv_moments(const float *adv, const int32_t *end, uint64_t n, const int32_t *segments,
                             uint32_t groups, double *moments, void *workspace, uint64_t workspace_bytes,
                             int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = ppo_groups_check(groups)) return rc;
    if (!segments || !moments || (n && !adv)) return fail(MBOTS_E_INVALID, "null argument");
    if (n > (uint64_t)INT32_MAX) return fail(MBOTS_E_INVALID, "more rows than a segment can name");
    const uint64_t chunks = pol_ppo_chunks(n, kPpoChunk);
    if (int rc = ppo_workspace_check(workspace, workspace_bytes, pol_ppo_bytes(chunks, groups))) return rc;
    if (device >= 0) {
        PolPpoIO io{};
        io.adv = adv, io.end = end, io.segments = segments, io.out = moments;
        io.part = static_cast<double *>(workspace), io.n = n, io.chunks = (uint32_t)chunks;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_adv_moments(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = segments_check_host(segments, groups, n, "rows")) return rc;
    for (uint32_t g = 0; g < groups; ++g)
        ppo_host_sum<kPpoMoments>(segments, g, kPpoChunk, moments + (size_t)kPpoMoments * g,
                                  [&](uint64_t r, double *acc) {
                                      if (!(end && end[r] == kTrajEndReset)) pol_ppo_moment_add(acc, adv[r]);
                                  });
    return MBOTS_OK;
}

int mbots_policy_ppo_loss(const float *logp, const float *value, const float *entropy, const float *old_logp,
                          const float *old_value, const float *adv, const float *ret, const int32_t *end, uint64_t n,
                          const int32_t *segments, uint32_t groups, const int64_t *rows, const double *moments,
                          float clip, float value_clip, float value_coef, float entropy_coef, float *g_logp,
                          float *g_value, float *g_entropy, double *stats, void *workspace, uint64_t workspace_bytes,
                          int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = ppo_groups_check(groups)) return rc;
    if (!segments || !rows) return fail(MBOTS_E_INVALID, "null segments or rows");
    if (n && (!logp || !value || !entropy || !old_logp || !adv || !ret)) return fail(MBOTS_E_INVALID, "null argument");
    if (n > (uint64_t)INT32_MAX) return fail(MBOTS_E_INVALID, "more rows than a segment can name");
    PpoCoef C;
    if (int rc = ppo_coef(clip, value_clip, old_value, value_coef, entropy_coef, C)) return rc;
    const uint64_t chunks = pol_ppo_chunks(n, kPpoChunk);
    if (int rc = ppo_workspace_check(workspace, workspace_bytes, pol_ppo_bytes(chunks, groups))) return rc;
    if (device >= 0) {
        const PolPpoIO io{logp, value, entropy, old_logp, old_value, adv, ret, end, segments, rows, moments, g_logp,
                          g_value, g_entropy, stats, static_cast<double *>(workspace), n, (uint32_t)chunks, C};
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_ppo_loss(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = segments_check_host(segments, groups, n, "rows")) return rc;
    for (float *o : {g_logp, g_value, g_entropy})
        if (o) std::fill(o, o + n, 0.0f);
    for (uint32_t g = 0; g < groups; ++g) {
        const float scale = pol_loss_scale(rows[g]);
        const PpoNorm N = pol_ppo_norm(moments ? moments + (size_t)kPpoMoments * g : nullptr);
        double sums[kPpoStats] = {};
        ppo_host_sum<kPpoStats>(segments, g, kPpoChunk, sums, [&](uint64_t r, double *acc) {
            const float w = (end && end[r] == kTrajEndReset ? 0.0f : 1.0f) * scale;
            float gl, gv, ge, st[kPpoStats];
            pol_ppo_row(logp[r], value[r], entropy[r], old_logp[r], C.vclip ? old_value[r] : 0.0f, adv[r], ret[r], w,
                        moments != nullptr, N, C, gl, gv, ge, st);
            if (g_logp) g_logp[r] = gl;
            if (g_value) g_value[r] = gv;
            if (g_entropy) g_entropy[r] = ge;
            for (uint32_t k = 0; k < kPpoStats; ++k) acc[k] += (double)st[k];
        });
        if (stats)
            for (uint32_t k = 0; k < kPpoStats; ++k) stats[(size_t)kPpoStats * g + k] += sums[k];
    }
    return MBOTS_OK;
}

int mbots_policy_seq_adv_moments(const float *adv, const int32_t *len, const int32_t *t0, const int32_t *end,
                                 uint32_t L, uint64_t B, const int32_t *order, const int32_t *segments,
                                 uint32_t groups, int32_t last_table, double *moments, void *workspace,
                                 uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (!moments) return fail(MBOTS_E_INVALID, "null argument");
    const int64_t none = 0;
    if (int rc = seq_loss_args(groups, B, len, t0, end, order, segments, &none)) return rc;
    if (L && B && !adv) return fail(MBOTS_E_INVALID, "null argument");
    if (L > (uint32_t)INT32_MAX) return fail(MBOTS_E_INVALID, "L is no int32 length");
    const uint64_t chunks = pol_ppo_chunks(B, kPpoSeqChunk);
    if (int rc = ppo_workspace_check(workspace, workspace_bytes, pol_ppo_bytes(chunks, groups))) return rc;
    if (device >= 0) {
        PolSeqPpoIO io{};
        io.adv = adv, io.len = len, io.t0 = t0, io.end = end, io.order = order, io.segments = segments;
        io.out = moments, io.part = static_cast<double *>(workspace), io.L = L, io.B = B;
        io.last_table = last_table, io.chunks = (uint32_t)chunks;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_seq_adv_moments(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = seq_loss_check_host(order, segments, groups, len, L ? L : 1u, B)) return rc;
    if (L == 0) return MBOTS_OK;
    for (uint32_t g = 0; g < groups; ++g)
        ppo_host_sum<kPpoMoments>(segments, g, kPpoSeqChunk, moments + (size_t)kPpoMoments * g,
                                  [&](uint64_t p, double *acc) {
                                      const int32_t b = order[p];
                                      const int32_t nk = pol_seq_kept(std::min(len[b], (int32_t)L), t0[b], end[b], last_table);
                                      for (int32_t k = 0; k < nk; ++k) pol_ppo_moment_add(acc, adv[(uint64_t)k * B + (uint32_t)b]);
                                  });
    return MBOTS_OK;
}

int mbots_policy_seq_ppo_loss(const float *logp, const float *value, const float *entropy, const float *old_logp,
                              const float *old_value, const float *adv, const float *ret, const int32_t *len,
                              const int32_t *t0, const int32_t *end, uint32_t L, uint64_t B, const int32_t *order,
                              const int32_t *segments, uint32_t groups, int32_t last_table, const int64_t *rows,
                              const double *moments, float clip, float value_clip, float value_coef,
                              float entropy_coef, float *g_logp, float *g_value, float *g_entropy, double *stats,
                              void *workspace, uint64_t workspace_bytes, int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = seq_loss_args(groups, B, len, t0, end, order, segments, rows)) return rc;
    if (L && B && (!logp || !value || !entropy || !old_logp || !adv || !ret))
        return fail(MBOTS_E_INVALID, "null argument");
    if (L > (uint32_t)INT32_MAX) return fail(MBOTS_E_INVALID, "L is no int32 length");
    PpoCoef C;
    if (int rc = ppo_coef(clip, value_clip, old_value, value_coef, entropy_coef, C)) return rc;
    const uint64_t chunks = pol_ppo_chunks(B, kPpoSeqChunk);
    if (int rc = ppo_workspace_check(workspace, workspace_bytes, pol_ppo_bytes(chunks, groups))) return rc;
    if (device >= 0) {
        const PolSeqPpoIO io{logp,  value,   entropy, old_logp, old_value, adv,     ret,       len,
                             t0,    end,     order,   segments, rows,      moments, g_logp,    g_value,
                             g_entropy, stats, static_cast<double *>(workspace), L, B, last_table, (uint32_t)chunks, C};
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_seq_ppo_loss(io, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    if (int rc = seq_loss_check_host(order, segments, groups, len, L ? L : 1u, B)) return rc;
    for (float *o : {g_logp, g_value, g_entropy})
        if (o) std::fill(o, o + (uint64_t)L * B, 0.0f);
    if (L == 0) return MBOTS_OK;
    for (uint32_t g = 0; g < groups; ++g) {
        if (rows[g] == 0) continue;   // the +0 stay, the statistics are not touched
        const float w = pol_loss_scale(rows[g]);
        const PpoNorm N = pol_ppo_norm(moments ? moments + (size_t)kPpoMoments * g : nullptr);
        double sums[kPpoStats] = {};
        ppo_host_sum<kPpoStats>(segments, g, kPpoSeqChunk, sums, [&](uint64_t p, double *acc) {
            const int32_t b = order[p];
            const int32_t nk = pol_seq_kept(std::min(len[b], (int32_t)L), t0[b], end[b], last_table);
            for (int32_t k = 0; k < nk; ++k) {
                const uint64_t r = (uint64_t)k * B + (uint32_t)b;
                float gl, gv, ge, st[kPpoStats];
                pol_ppo_row(logp[r], value[r], entropy[r], old_logp[r], C.vclip ? old_value[r] : 0.0f, adv[r], ret[r],
                            w, moments != nullptr, N, C, gl, gv, ge, st);
                if (g_logp) g_logp[r] = gl;
                if (g_value) g_value[r] = gv;
                if (g_entropy) g_entropy[r] = ge;
                for (uint32_t q = 0; q < kPpoStats; ++q) acc[q] += (double)st[q];
            }
        });
        if (stats)
            for (uint32_t k = 0; k < kPpoStats; ++k) stats[(size_t)kPpoStats * g + k] += sums[k];
    }
    return MBOTS_OK;
}

int mbots_policy_ppo_gate(const double *stats, const int64_t *rows, uint32_t groups, double target_kl, int64_t *gate,
                          int32_t device, void *stream)
{
    using namespace mbots;
    if (int rc = ppo_groups_check(groups)) return rc;
    if (!stats || !rows || !gate) return fail(MBOTS_E_INVALID, "null argument");
    if (device >= 0) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_policy_ppo_gate(stats, rows, target_kl, gate, groups, as_stream(stream)));
        return MBOTS_OK;
    }
    for (uint32_t g = 0; g < groups; ++g)
        gate[g] = pol_ppo_gate(gate[g], rows[g], stats[(size_t)kPpoStats * g + 4u], target_kl);
    return MBOTS_OK;
}

}  // extern "C"
