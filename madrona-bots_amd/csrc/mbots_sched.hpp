// The step's cross-queue ordering: which queue waits for which before a kernel
// may touch a buffer two queues share ("Schedule").  Host logic
// only, no HIP: queues, events and signal words are named by index, a graph
// capture by an opaque id (0: none), a caller's stream by an opaque pointer,
// and every runtime call goes through an executor the caller passes in.  The
// manager (mbots_manager.cpp) keeps the HIP objects in arrays under the same
// indices; tests/c_host/sched_model.cpp runs the same rules over a symbolic
// executor and checks happens-before for every call order.
//
// The executor (any type with these members; the int ones return 0 or an
// error code, which the rule passes up at once):
//   caller()                 the call's stream, as an opaque pointer
//   record(ev, q)            record event ev on queue q
//   wait_event(q, ev)        queue q waits for event ev
//   wait_value(q, sig, e)    queue q waits for signal word sig >= e
//   raise_join(e)            a one-wave store of e to the join word, on the
//                            sensor's queue (after the sensor)
//   pending(ev)              is event ev's last record still not reached?
//   drain_and_zero()         the device drained, both signal words zeroed
//   capture_of(q, id)        id = the capture queue q is being recorded into
//   refuse(why, n)           the error code of a refusal (and its message)
#pragma once
#include <algorithm>
#include <cstdint>

namespace mbots {
namespace sched {

// queues: the call's stream, the sensor's internal stream, the stream of the
// manager's last call, the stream the last captured step was recorded on
constexpr int kCaller = 0, kSensor = 1, kLast = 2, kCapture = 3;
// events: the sensors of alternate steps, K2's row counts, the caller's stream
// at a swapped step's start, the hop between two caller streams
constexpr int kJoin0 = 0, kJoin1 = 1, kTotals = 2, kCallerEv = 3, kHop = 4, kNumEvents = 5;
// signal words: K2's last block raises the fork, a wave after the sensor the join
constexpr int kFork = 0, kJoin = 1;
enum Refusal {
    kPoisoned,          // a graph of an odd number of steps was captured
    kCaptureElsewhere,  // a capture of this manager's steps still records on another stream
    kOddJoin,           // join() inside a capture after an odd number of steps (n: the count)
};

// The fork (K2 -> the sensor's queue) as a value wait on a flag K2's last
// block stores, instead of a wait on K2's completion signal: the hop is ~3 us
// instead of ~7 (scripts/ubench/hop_latency.hip).  At small world counts the
// step is a latency chain and that is -1 to -4 % at 4096 worlds; from 16384 on
// the chip is throughput-bound from K1's end on and the flag's fences cost
// about what the hop saves (±0 at 16384, +0.2-0.6 % at 65536), so events there
// (profiles/r04_value_fork_small_ab.jsonl, profiles/r04_value_waits_ab.jsonl,
// DESIGN_EXPERIMENTS.md round 4).
#ifndef MB_VALUE_FORK_MAX
#define MB_VALUE_FORK_MAX 8192
#endif
#ifndef MB_VALUE_JOIN
#define MB_VALUE_JOIN 1   // the join too: a one-wave kernel after the sensor raises it
#endif
#ifndef MB_VALUE_JOIN_MAX
#define MB_VALUE_JOIN_MAX 8192
#endif
#ifndef MB_SWAP_DEFAULT
#define MB_SWAP_DEFAULT 1   // MBOTS_SWAP's default (large world counts)
#endif
#ifndef MB_VALUE_ADAPT
#define MB_VALUE_ADAPT 1   // value waits only while the host runs ahead of the device
#endif
// Up to this many worlds K1 computes the next step's finder slots itself
// (world_finders), so the next K1 waits only for the caller's stream, not for
// this step's sensor: the sensor chain and the caller chain of consecutive
// steps overlap ("Schedule")
#ifndef MB_FINDER_AUX_LOW
#define MB_FINDER_AUX_LOW 0
#endif
#ifndef MB_K1_FINDER_MAX
#define MB_K1_FINDER_MAX 2048
#endif
// the value waits' epochs restart from 0 once they reach this (before_k2)
constexpr uint32_t kEpochWrap = 0x7FFFFFF0u;

// the environment's part of the choice (read once, at create)
struct Knobs {
    // MBOTS_VALUE_FORK is not 0 and no serialising tool is set.  (The runtime
    // carries a value wait as a polling kernel on the sensor's queue, which
    // spins until K2 on the caller's queue raises the flag: under a tool that
    // runs the device's kernels one at a time the poller can be dispatched
    // first and never end.)
    bool value_waits_safe = true;
    int swap = -1;   // MBOTS_SWAP: 0, 1, or -1 when unset
};

// The four schedules: forked with event waits (none of the four set), forked
// with value waits (value_fork / value_join, each where its signal word could
// be allocated), K1-finder, swapped
struct Mode {
    bool k1_finder = false;    // K1 computes the finder slots: the next K1 does not wait for the sensor
    bool value_fork = false;   // the sensor's queue waits for K2's flag
    bool value_join = false;   // the next K1 waits for the flag raised after the sensor
    bool swap = false;         // K1 and K2 on the sensor's queue, the caller's joining after K2
    bool values() const { return value_fork || value_join; }
    bool aux_low() const { return k1_finder && MB_FINDER_AUX_LOW; }   // the sensor's queue is the filler
};

// (the K1 finder pass keeps camera slots in bytes: a <= 256-slot mode.
// K1-finder mode takes event forks: the caller's chain no longer waits for the
// sensor, and the value fork's 5.5 us enqueue lands on that chain's host time;
// an event fork measured -5 % at 2048 worlds.  The swap is the default above
// 8192 worlds since round 6: with the prev-sensor move lazy the caller's chain
// is the shorter one from the first steps on, and the swap takes both hops off
// the sensor's chain: -1.9 % in the driver's window, -2.1 % at steady state,
// interleaved on one box; MBOTS_SWAP=0 restores the forked schedule)
inline Mode choose(uint64_t worlds, uint32_t capacity, bool fork_mem, bool join_mem, const Knobs &k)
{
    Mode m;
    m.k1_finder = worlds <= MB_K1_FINDER_MAX && capacity <= 256;
    const bool small = worlds > MB_K1_FINDER_MAX && k.value_waits_safe;
    m.value_fork = fork_mem && small && worlds <= MB_VALUE_FORK_MAX;
    m.value_join = join_mem && small && MB_VALUE_JOIN && worlds <= MB_VALUE_JOIN_MAX;
    const bool want = k.swap >= 0 ? k.swap == 1 : MB_SWAP_DEFAULT != 0;
    m.swap = want && worlds > MB_VALUE_FORK_MAX && !m.k1_finder && !m.values();
    return m;
}

// what a step's launches need of the schedule
struct Step {
    unsigned long long capture = 0;   // the capture the step is recorded into
    bool plain_records = false;       // ... so the fork / join events are plain records
    bool ahead = false;    // the host reached this step while the last sensor still ran
    int kq = kCaller;      // the queue of the reset pass, K1 and K2
    uint32_t epoch = 0;    // this step's epoch (0: event waits)
    uint32_t k2_epoch = 0; // ... as K2's last block raises it (0: it raises none)
    int join = kJoin0;     // the event this step's sensor is recorded in
};

struct Schedule {
    Mode mode;
    Knobs knobs;
    int last_join = -1;               // the join event of the latest sensor, -1: none pending
    unsigned long long join_capture = 0;   // the capture it was recorded in (0: none)
    int prev_join = -1;               // the event of the sensor before it (its rows are the
    unsigned long long prev_capture = 0;   // other table half's), -1: none
    uint64_t join_serial[2] = {0, 0}; // the sensor launch (1, 2, ...) each join event marks
    uint64_t sensor_serial = 0;       // sensors launched
    uint64_t waited_serial = 0;       // the newest sensor the manager's stream order has waited
                                      // for (outside graph capture; every call follows the last)
    uint32_t epoch = 0;               // the last epoch K2 raised (never 0)
    uint32_t epoch_wraps = 0;         // times the epochs restarted from 0 (kEpochWrap)
    uint32_t join_epoch = 0;          // the epoch raised after the last sensor (0: none; the
                                      // join is then the sensor's event)
    const void *last_stream = nullptr;   // the stream of the manager's last call
    unsigned long long cap_seen = 0;  // the capture the last captured step belonged to
    const void *cap_stream = nullptr; // the stream it was recorded on (live while capturing)
    uint64_t cap_steps = 0;           // steps recorded into it (join wants an even count)
    bool poisoned = false;            // a graph of an odd number of steps was captured: the
                                      // host's table bookkeeping no longer follows the device

    bool graph_exists() const { return cap_seen != 0; }
    bool sensor_launched() const { return last_join >= 0; }
    // mbots_schedule_info's mode bits (1 2 4 8), epoch and wraps
    uint32_t info_bits() const
    {
        return (mode.k1_finder ? 1u : 0u) | (mode.value_fork ? 2u : 0u) | (mode.value_join ? 4u : 0u) |
               (mode.swap ? 8u : 0u);
    }

    // A graph captured with an odd number of steps leaves the table halves and
    // the host's deferred-move bookkeeping out of step with the device after a
    // replay: every device entry point refuses to run from then
    // on.  (only a capture that has ENDED with an odd count poisons;
    // a call on another stream while the capture is still recording is refused
    // alone.)  q: the queue the call is made on, -1: outside any capture
    template <class Ex> int guard(Ex &ex, int q)
    {
        if (poisoned) return ex.refuse(kPoisoned, 0);
        if ((cap_steps & 1) && (q < 0 || !capture(ex, q))) {
            if (cap_stream && cap_seen && capture(ex, kCapture) == cap_seen) return ex.refuse(kCaptureElsewhere, 0);
            poisoned = true;
            return ex.refuse(kPoisoned, 0);
        }
        return 0;
    }

    // Every call enqueues on the caller's stream; a call on another stream than
    // the previous one is ordered after everything the manager enqueued there
    // (an event hop), so steps, deferred copies and the views they produce form
    // one stream-ordered sequence whatever streams the caller switches between.
    // (Not across a graph capture's boundary: a capture cannot wait for work
    // outside it.)
    template <class Ex> int enter(Ex &ex)
    {
        if (int rc = guard(ex, kCaller)) return rc;
        if (ex.caller() != last_stream && !capture(ex, kCaller) && !capture(ex, kLast)) {
            if (int rc = ex.record(kHop, kLast)) return rc;
            if (int rc = ex.wait_event(kCaller, kHop)) return rc;
        }
        last_stream = ex.caller();
        return 0;
    }

    // make the caller's stream wait for the last step's sensor (its rows, and
    // the moves it did)
    template <class Ex> int wait_sensor(Ex &ex) { return wait_last(ex, kCaller, false); }

    // make the caller's stream wait for the sensor before the last one, whose
    // rows are the other table half's (the prev-sensor moves read them).  Only
    // needed when K1 does not wait for the sensors (K1-finder): otherwise the
    // last step's K1 did.  (Under stream capture, only an event recorded in the
    // same capture.)
    template <class Ex> int wait_prev_sensor(Ex &ex)
    {
        if (!mode.k1_finder || prev_join < 0) return 0;
        unsigned long long cap = 0;
        if (int rc = ex.capture_of(kCaller, cap)) return rc;
        if (cap && prev_capture != cap) return 0;
        // (one cross-queue wait per step: the shift's for its prev-sensor rows
        // covers the next K1's)
        if (!cap && waited_serial >= join_serial[prev_join]) return 0;
        if (int rc = ex.wait_event(kCaller, prev_join)) return rc;
        if (!cap) waited_serial = std::max(waited_serial, join_serial[prev_join]);
        return 0;
    }

    // join(): the caller's stream after the last sensor.  The table halves and
    // the host's deferred-move bookkeeping alternate per step: a graph of an odd
    // number of steps would leave them out of step with the device after every
    // replay
    template <class Ex> int join(Ex &ex)
    {
        if (int rc = enter(ex)) return rc;
        unsigned long long cap = 0;
        if (int rc = ex.capture_of(kCaller, cap)) return rc;
        if (cap && cap == cap_seen && (cap_steps & 1)) return ex.refuse(kOddJoin, cap_steps);
        if (last_join >= 0) return ex.wait_event(kCaller, last_join);
        return 0;
    }

    // a restore: no sensor is outstanding and the device is idle
    void idle_reset()
    {
        last_join = -1;
        prev_join = -1;
        waited_serial = sensor_serial;
        join_epoch = 0;
        last_stream = nullptr;
    }

    // The step's edges, in order.  First the capture's bookkeeping and the
    // entry on the caller's stream (a new capture: the previous one must have
    // held an even number of steps)
    template <class Ex> int begin_step(Ex &ex, Step &s)
    {
        s = Step{};
        if (int rc = ex.capture_of(kCaller, s.capture)) return rc;
        s.plain_records = s.capture != 0;
        if (s.capture && s.capture != cap_seen) {
            if (int rc = guard(ex, -1)) return rc;
            cap_seen = s.capture;
            cap_stream = ex.caller();
            cap_steps = 0;
        }
        if (int rc = enter(ex)) return rc;
        if (s.capture) ++cap_steps;
        return 0;
    }

    // What K1's queue waits for.  K1 reads the finder slots the previous step's
    // sensor wrote, and writes the state half that sensor read.  (Under stream
    // capture only a join recorded in the same capture is waited for: a replay
    // starts after the previous launch of the graph completed.)  Value waits:
    // eagerly, while the device still runs the previous step, the flag a wave
    // after the sensor raised.  A host that arrives after the sensor has
    // finished -- a host-bound loop, where the value waits' extra enqueues would
    // only add host time -- takes the event wait, and this step raises no flags.
    template <class Ex> int before_k1(Ex &ex, Step &s)
    {
        const bool capturing = s.capture != 0;
        if (!capturing && mode.values()) s.ahead = !MB_VALUE_ADAPT || last_join < 0 || ex.pending(last_join);
        // swapped: K1, K2 and the sensor on the internal queue with no hop
        // between them; K1 after the last sensor (the same queue) and after what
        // the caller enqueued so far (the learner's writes)
        if (mode.swap && !capturing) {
            s.kq = kSensor;
            if (int rc = ex.record(kCallerEv, kCaller)) return rc;
            return ex.wait_event(kSensor, kCallerEv);
        }
        // K1-finder: K1 computed the finder slots this K1 reads; it must only not
        // overwrite the state half the sensor before the last one may still read
        if (mode.k1_finder) return wait_prev_sensor(ex);
        // ">=" (VERDICT r5 item 5): the flag only grows -- one writer, raised in
        // step order on the sensor's queue -- so this wait passes whenever it is
        // reached, even after a later step has raised the flag again; an
        // equality wait would hang there (the round-5 probe's fork did)
        if (!capturing && join_epoch != 0 && s.ahead) return ex.wait_value(kCaller, kJoin, join_epoch);
        return wait_last(ex, kCaller, true);
    }

    // The reset pass runs before K1 on K1's queue and after K1's waits: it
    // writes the state half K1 reads, whose finder slots the last sensor wrote,
    // and reads the flags the caller's stream wrote.  In K1-finder mode K1 does
    // not wait for that sensor, which still reads this half: the pass does
    template <class Ex> int before_reset_pass(Ex &ex, const Step &s)
    {
        return mode.k1_finder ? wait_last(ex, s.kq, true) : 0;
    }

    // This step's epoch: K2's last block raises it (under capture replays would
    // repeat it: the event then).  Both waits are "flag >= epoch": before the
    // counter wraps, drain the device and restart both from 0 -- the resets
    // complete before any later wait is enqueued (exercised by
    // tests/test_robustness.py::test_value_wait_epoch_wrap through
    // MBOTS_EPOCH_START)
    template <class Ex> int before_k2(Ex &ex, Step &s)
    {
        if (mode.values() && !s.capture && s.ahead) {
            if (epoch >= kEpochWrap) {
                if (int rc = ex.drain_and_zero()) return rc;
                epoch = 0;
                join_epoch = 0;
                ++epoch_wraps;
            }
            s.epoch = ++epoch;
        }
        s.k2_epoch = mode.value_fork ? s.epoch : 0u;
        return 0;
    }

    // Who waits for K2.  The sensor (it derives the export rows from K2's row
    // bases itself) runs on its own queue while the caller's goes on with K3a,
    // shift_observations and the learner's action writes -- none of which reads
    // the sensor rows or the finder slots.  Swapped, the caller's queue joins
    // here instead.  (">=": the fork flag only grows -- K2's last block raises
    // each step's epoch in step order -- so the wait passes whenever the
    // sensor's queue reaches it, also after a later K2 raised the flag again;
    // equality would hang there)
    template <class Ex> int before_sensor(Ex &ex, Step &s)
    {
        s.join = last_join == 0 ? kJoin1 : kJoin0;
        if (s.kq == kSensor) return ex.wait_event(kCaller, kTotals);
        if (s.epoch && mode.value_fork) return ex.wait_value(kSensor, kFork, s.epoch);
        return ex.wait_event(kSensor, kTotals);
    }

    // the sensor is enqueued (its join event rides its dispatch): the next K1
    // and the sensor rows' readers wait for it
    template <class Ex> int after_sensor(Ex &ex, const Step &s)
    {
        join_serial[s.join] = ++sensor_serial;
        prev_join = last_join;
        prev_capture = join_capture;
        last_join = s.join;
        join_capture = s.capture;
        join_epoch = 0;
        if (s.epoch && mode.value_join) {
            if (int rc = ex.raise_join(s.epoch)) return rc;
            join_epoch = s.epoch;
        }
        return 0;
    }

private:
    template <class Ex> static unsigned long long capture(Ex &ex, int q)
    {
        unsigned long long id = 0;
        return ex.capture_of(q, id) ? 0 : id;   // (a stream the runtime cannot query records nothing)
    }

    // queue q waits for the last sensor's event; same_capture: inside a capture
    // only when the event was recorded in it
    template <class Ex> int wait_last(Ex &ex, int q, bool same_capture)
    {
        if (last_join < 0) return 0;
        const unsigned long long cap = capture(ex, kCaller);
        if (same_capture && cap && join_capture != cap) return 0;
        if (int rc = ex.wait_event(q, last_join)) return rc;
        if (!cap) waited_serial = std::max(waited_serial, join_serial[last_join]);
        return 0;
    }
};

}  // namespace sched
}  // namespace mbots
