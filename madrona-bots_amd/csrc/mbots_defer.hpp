// The manager's deferred columns: which columns of the two observation-table
// halves are owed instead of written, and the rules that make them real in
// time ("Lazy shift" ... "Owed PrevAction").  Host logic only, no
// HIP: every buffer is named by an index (a table half, one of the two
// PrevHiddenState storages, a step parity's src_of / map / row-count word) and
// the device work goes through an executor the caller passes in.  The manager
// (mbots_manager.cpp) turns indices into pointers; tests/c_host/defer_model.cpp
// runs the same rules over symbolic tables against an eager reference.
//
// The executor (any type with these members; each returns 0 or an error code,
// which the rule passes up at once):
//   move(part, six_lazy)    launch_move of one kPart* from the last half into
//                           the current one along the last step's src_of (the
//                           source's Action / HiddenState through its view)
//   move_shift(word)        the fused shift: PrevAction / PrevHiddenState of
//                           the current half from the last half's view; with
//                           word >= 0 PrevAction alone, the row count stored
//                           in that word
//   shift(rest)             launch_shift over the current half: Action /
//                           HiddenState to their Prev columns, or (rest) the
//                           six other columns
//   gather_hidden(half, map, base_half, word, exchange)
//                           half's PrevHiddenState = base[map[r]] over *word
//                           rows, base the PrevHiddenState storage base_half
//                           holds (after the two halves exchanged theirs, if
//                           asked); then *word = 0
//   gather_prev_action(half, par, base_prev)
//                           half's PrevAction = base[src_of[par][r]] over the
//                           PrevAction word of par; base the other half's
//                           PrevAction (base_prev) or Action storage; then the
//                           word = 0
//   copy_out(action, hidden)   the current half's aliased columns copied from
//                           their Prev storages
//   wait_prev_sensor()      the stream waits for the sensor before the last
#pragma once
#include <utility>

namespace mbots {
namespace defer {

// the columns a caller names (require)
constexpr int kAction = 1, kHidden = 2, kPrevAction = 4, kPrevHidden = 8, kPrev6 = 16, kPrevSensor = 32;
// the parts of a step's row move (launch_move's masks: the manager asserts
// they are mbots_kernels.hpp's kMove*)
constexpr int kPartAH = 1, kPartSensor = 4, kPartPrevAH = 8, kPartPrev6 = 16;
constexpr int kOwnWord = 4;   // the row-count word a lazy shift's own launch stores

enum class How {
    Rows,        // reads the columns' real rows in their storages (accessors,
                 // set_action, the trajectory push, records)
    View,        // goes through the half's view (K1, the device actor): the
                 // step's owed move is made, an aliased column stays one
    WriteAll,    // rewrites every live row
    WritePart,   // writes some rows: the others are kept
};

struct Env {
    bool capturing = false;       // the call's stream is being captured
    bool graph_exists = false;    // a graph of this manager's steps exists
    bool pa_on = true;            // owed PrevAction enabled
    bool psem_by_sensor = false;  // K1-finder mode: the sensor moves the prev sensor
};

// what a step needs of the state (begin_step) and hands back (end_step)
struct StepPlan {
    int lazy = 0;            // the prefetch move's six_lazy argument
    int prefetch = 0;        // kPart* moved right after this step's K3a
    int map_in = -1;         // the map buffer K3a composes from (parity), -1: src_of itself
    int map_out = -1;        // ... and writes (this parity), -1: none
    bool map_plain = false;  // it stores src_of as its map
    bool store_rows = false; // K2 stores the row counts for the owed gathers
};

// deferred K4 parts of a table half (moved from the other half along the last
// src_of when needed), and what a shift left as views
struct Half {
    bool cur_ah_owed = false;   // Action / HiddenState themselves
    bool psem_owed = false;     // the prev sensor (moved only when read: dead at the next step)
    bool prev_ah_owed = false;  // PrevAction / PrevHiddenState
    bool six_owed = false;      // the six other Prev* columns ...
    bool six_lazy = false;      // ... from the other half's current ones
    // the half's current Action / HiddenState column is its Prev column: a
    // fused shift gathered the moved rows into PrevAction / PrevHiddenState only
    // (the learner overwrites the current ones next); readers go through the
    // view, accessors copy first
    bool a_alias = false, h_alias = false;
    bool prev_lazy = false;     // the six shift-owned Prev* columns are still the current ones (lazy shift)
};

struct Deferred {
    Half half[2];
    int tb = 0;        // the current table half
    int parity = 0;    // the next step's buffers
    // which PrevHiddenState storage each half holds (ending lazy HiddenState
    // may exchange them)
    int ph_store[2] = {0, 1};
    // lazy HiddenState: half hid_half's PrevHiddenState storage holds nothing;
    // the column is base[map[r]] (0 where map[r] < 0), base the storage
    // hid_base, map the buffer of parity hid_map that K3a composes every step,
    // over the rows in word hid_word; while h_alias[hid_half] holds HiddenState
    // is that too.  The base is not written while the state holds.  The lazy
    // half is the current one after a lazy shift and the last one after a step
    bool hid_lazy = false;
    int hid_half = 0, hid_map = 0, hid_base = 0, hid_word = kOwnWord;
    bool hid_map_plain = false;   // the last step stored src_of as its map (it ran not lazy):
                                  // the map a stretch may begin with
    // owed PrevAction: half pa_half's PrevAction storage holds nothing; the
    // column is base[src_of[pa_par][r]] (0 where < 0) over the rows in the
    // PrevAction word of pa_par, base the last half's Action as the shift saw
    // it -- its PrevAction storage (pa_base_prev) when that was aliased; while
    // a_alias[pa_half] holds Action is that too.  Neither base nor src_of is
    // written while the state holds
    bool pa_lazy = false;
    int pa_half = 0, pa_par = 0;
    bool pa_base_prev = false;
    int src_par = -1;    // the parity whose src_of buffer the last step wrote (-1: none since reset)
    int forced = 0;      // parts the caller's reads needed since the last step: the next step prefetches them
    int prefetched = 0;  // parts this step prefetched and no shift superseded

    // a checkpoint load / a growth: nothing is deferred
    void reset()
    {
        const int s0 = ph_store[0], s1 = ph_store[1];   // (the storages stay where they are)
        *this = Deferred{};
        ph_store[0] = s0;
        ph_store[1] = s1;
    }

    const Half &cur() const { return half[tb]; }
    // readers of the current half's six shift-owned Prev* columns
    bool prev_is_current() const { return half[tb].prev_lazy; }   // they are still its current ones
    bool six_owed() const { return half[tb].six_owed; }            // ... or owed: gathered from the last half
    bool six_lazy() const { return half[tb].six_lazy; }            //     (its current ones)
    bool psem_owed() const { return half[tb].psem_owed; }
    bool action_aliased(int h) const { return half[h].a_alias; }
    bool hidden_aliased(int h) const { return half[h].h_alias; }
    bool hidden_lazy() const { return hid_lazy; }
    bool prev_action_owed() const { return pa_lazy; }
    // the half whose PrevHiddenState storage is `store`
    int holder(int store) const { return ph_store[0] == store ? 0 : 1; }

    // a caller reads or writes `cols` of the current half
    template <class Ex> int require(Ex &ex, int cols, How how)
    {
        const int owed = owed_parts();
        int need = 0;
        if (cols & kPrev6) {
            need |= kPartPrev6;
            if (int rc = settle_prev6(ex)) return rc;
        }
        if (cols & (kPrevAction | kPrevHidden)) {
            need |= kPartPrevAH;
            if (cols & kPrevHidden)
                if (int rc = end_hidden(ex)) return rc;
            if (cols & kPrevAction)
                if (int rc = end_prev_action(ex)) return rc;
            if (int rc = settle_prev_ah(ex)) return rc;
        }
        if (cols & (kAction | kHidden)) {
            need |= kPartAH;
            // a reader of rows, or a writer that keeps some, finds an aliased
            // column copied out of its Prev storage; a column written whole is
            // simply written, a view reads the Prev storage
            const int out = how == How::Rows || how == How::WritePart ? cols & (kAction | kHidden) : 0;
            if (int rc = settle_cur_ah(ex, out)) return rc;
            // (a lazy HiddenState column a net reads through the view: real rows
            // in the Prev storage first)
            if (how == How::View && (cols & kHidden) && half[tb].h_alias)
                if (int rc = end_hidden(ex)) return rc;
            if (how == How::WriteAll || how == How::WritePart) {
                if (cols & kAction) half[tb].a_alias = false;
                if (cols & kHidden) half[tb].h_alias = false;
            }
        }
        if (cols & kPrevSensor) {
            need |= kPartSensor;
            if (int rc = settle_psem(ex)) return rc;
        }
        note_use(need, owed);
        return 0;
    }

    // every column of the current half real in its storage (the learner pack,
    // whose reads are remembered for the next step's prefetch: `hint`; a
    // checkpoint save; a growth)
    template <class Ex> int require_all(Ex &ex, bool hint)
    {
        const int owed = owed_parts();
        if (int rc = end_hidden(ex)) return rc;
        if (int rc = end_prev_action(ex)) return rc;
        if (int rc = settle_prev6(ex)) return rc;
        if (int rc = settle_prev_ah(ex)) return rc;
        if (int rc = settle_cur_ah(ex, kAction | kHidden)) return rc;
        if (int rc = settle_psem(ex)) return rc;
        if (hint) note_use(kPartPrev6 | kPartPrevAH | kPartAH | kPartSensor, owed);
        return 0;
    }

    // an owed PrevAction made real on its own (mbots_reset_worlds)
    template <class Ex> int require_prev_action_storage(Ex &ex) { return end_prev_action(ex); }

    // the top of a step: what the last step still owes the current half that
    // this step's K1 and moves read, and the plan of this step
    template <class Ex> int begin_step(Ex &ex, const Env &env, StepPlan &plan)
    {
        const int par = parity;
        plan = StepPlan{};
        plan.lazy = half[tb].prev_lazy ? 1 : 0;
        // the parts the caller's reads forced last step (a learner that reads the
        // observation and PrevHiddenState between step and shift, as
        // training_loop.py:47-88 does): moved right after this step's K3a, beside
        // the sensor, instead of behind the wait for it (DESIGN.md "Prefetch")
        const int prefetch = forced;
        forced = 0;
        prefetched = prefetch;
        // lazy HiddenState goes on only from a shift (the lazy half is then the
        // current one, its map the last step's): after a step with no shift, before
        // a prefetch of Action / HiddenState or their Prev columns, and under
        // stream capture (a replay must not depend on the host's lazy state) it
        // is materialised first
        if (hid_lazy && (hid_half != tb || hid_map == par || env.capturing || (prefetch & (kPartAH | kPartPrevAH))))
            if (int rc = end_hidden(ex)) return rc;
        // owed PrevAction likewise goes on only from a shift whose Action a
        // whole-table writer has replaced since (else K1 reads the owed view), and
        // never into the step whose K3a and K2 write the src_of buffer and the row
        // count it holds (a shift in between has made it dead; not assumed)
        if (pa_lazy && (pa_half != tb || half[tb].a_alias || pa_par == par || env.capturing ||
                        (prefetch & (kPartAH | kPartPrevAH))))
            if (int rc = end_prev_action(ex)) return rc;
        // no shift since the last step: its deferred Prev moves first
        if (half[tb].six_owed)
            if (int rc = settle_prev6(ex)) return rc;
        if (int rc = settle_prev_ah(ex)) return rc;
        if (int rc = settle_cur_ah(ex, 0)) return rc;
        // (a prev sensor still owed is dead from here on: the new table's prev
        // sensor is the last table's sensor rows, updateSensorOutputIdx
        // sim.cpp:736-789, not its prev sensor -- so it is never moved)
        // (the prev sensor is the sensor's own part in K1-finder mode)
        plan.prefetch = env.psem_by_sensor ? prefetch & ~kPartSensor : prefetch;
        // K3a composes the row map of lazy HiddenState into this step's buffer from
        // the last step's (the other one: the lazy half's map stays readable until
        // the next shift moves on to this one); not lazy, it stores src_of there,
        // the map a lazy shift begins a stretch with -- only where the next shift
        // could begin one: HiddenState is a view now (nothing but a shift makes it
        // one), so a loop that writes memory every step stores no map
        const bool map_wanted = hid_lazy || (half[tb].h_alias && !env.graph_exists && !env.capturing);
        plan.map_out = map_wanted ? par : -1;
        plan.map_in = hid_lazy ? hid_map : -1;
        plan.map_plain = map_wanted && !hid_lazy;
        // (owed PrevAction on: K2 also stores the table's rows where the gathers of
        // the owed columns read them -- the shift that follows launches nothing.
        // Not where a graph could replay the store over a count still in use)
        plan.store_rows = env.pa_on && !env.graph_exists && !env.capturing;
        return 0;
    }

    // the step is enqueued: the halves swap, and the new half's Prev* columns
    // are eight moves deferred (a shift overwrites them) but for the prefetched
    void end_step(const StepPlan &plan, bool psem_by_sensor)
    {
        hid_map_plain = plan.map_plain;
        src_par = parity;
        parity ^= 1;
        tb ^= 1;
        Half &n = half[tb];
        n = Half{};
        n.cur_ah_owed = !(plan.prefetch & kPartAH);
        n.psem_owed = !psem_by_sensor && !(plan.prefetch & kPartSensor);
        n.prev_ah_owed = !(plan.prefetch & kPartPrevAH);
        n.six_owed = !(plan.prefetch & kPartPrev6);
        n.six_lazy = plan.lazy != 0;
    }

    // shift_observations.  Action / HiddenState now; the other six Prev*
    // columns stay views of the current ones until the next step or an accessor
    // needs them (lazy shift).  Action / HiddenState still in the other half: one
    // gather writes their Prev copies, and the current columns become views of
    // those (the learner overwrites them next; DESIGN.md "Aliased current Action
    // / HiddenState") -- the fused shift.  The step's prev-sensor move is not
    // the shift's (shiftObservationsSystem, sim.cpp:1001-1035, leaves the sensor
    // alone): it stays owed until a reader needs it and dies at the next step
    // (DESIGN.md "Lazy prev sensor").
    template <class Ex> int shift(Ex &ex, const Env &env)
    {
        Half &c = half[tb];
        const Half &l = half[tb ^ 1];
        const bool fused = c.cur_ah_owed;
        // Lazy HiddenState (DESIGN.md "Lazy HiddenState"): the last half's
        // HiddenState is still only a view -- of its PrevHiddenState storage (a
        // fused shift's: nobody copied it out or wrote it since), or of the lazy
        // column -- so this half's HiddenState / PrevHiddenState are those rows
        // along src_of: not gathered but owed, as (base, composed map).  The base
        // is that storage on entry and stays while the state goes on.  Not under
        // stream capture, nor once a graph of this manager's steps exists (its
        // replays read the columns in the storages they recorded).
        const bool old_lazy = hid_lazy && hid_half == (tb ^ 1);
        const bool lazy = fused && l.h_alias && !env.graph_exists && !env.capturing &&
                          (old_lazy || (!hid_lazy && hid_map_plain));
        if (fused && hid_lazy && !lazy) {
            // the last half's lazy PrevHiddenState: the source of HiddenState here
            // while that is its view; else dead (this shift overwrites what derives
            // from it), and its base is free again
            if (l.h_alias) {
                if (int rc = end_hidden(ex)) return rc;
            } else {
                hid_lazy = false;
            }
        }
        // Owed PrevAction (DESIGN.md "Owed PrevAction"): the last half's owed
        // column is the source of Action here while that is still its view (nobody
        // wrote it: real rows first); else it is dead -- this shift supersedes the
        // Prev move that would have read it -- and its base and src_of are free
        if (fused && pa_lazy) {
            if (pa_half != (tb ^ 1) || l.a_alias) {
                if (int rc = end_prev_action(ex)) return rc;
            } else {
                pa_lazy = false;
            }
        }
        int rc = 0;
        if (fused) {
            const int last = parity ^ 1;   // the last step's buffers
            // the launch would gather Action alone: PrevAction (and Action, its
            // view) owed as (that Action, the last step's src_of) instead, and no
            // launch at all -- K2 stored both row counts
            const bool owe = lazy && env.pa_on && src_par == last;
            if (lazy) hid_word = owe ? last : kOwnWord;
            if (!owe) rc = ex.move_shift(lazy ? hid_word : -1);
            if (rc == 0 && lazy) {
                if (!old_lazy) hid_base = ph_store[tb ^ 1];
                hid_lazy = true;
                hid_half = tb;
                hid_map = last;
            }
            if (owe) {
                pa_lazy = true;
                pa_half = tb;
                pa_base_prev = l.a_alias;
                pa_par = last;
            }
        } else if (!(c.a_alias && c.h_alias)) {   // both aliased: already equal
            if ((rc = settle_cur_ah(ex, kAction | kHidden))) return rc;
            // (HiddenState was written since a lazy shift: the lazy PrevHiddenState
            // is overwritten here)
            if (hid_lazy && hid_half == tb) hid_lazy = false;
            // (... and Action since an owed shift: so is the owed PrevAction)
            if (pa_lazy && pa_half == tb) pa_lazy = false;
            rc = ex.shift(false);
        }
        if (rc == 0) {
            // Action / HiddenState and every Prev* column but the sensor's are the
            // shift's now: a later read of them is not the step's deferred move
            prefetched &= kPartSensor;
            if (fused) c.a_alias = c.h_alias = true;
            c.cur_ah_owed = false;
            c.prev_lazy = true;
            c.prev_ah_owed = false;   // the shift wrote PrevAction / PrevHiddenState
            c.six_owed = false;       // ... and made the six the current columns
        }
        return rc;
    }

private:
    // deferred parts still owed by the current half
    int owed_parts() const
    {
        const Half &c = half[tb];
        return (c.cur_ah_owed ? kPartAH : 0) | (c.psem_owed ? kPartSensor : 0) | (c.prev_ah_owed ? kPartPrevAH : 0) |
               (c.six_owed ? kPartPrev6 : 0);
    }
    // a caller's read that needs the parts `need`: the ones the step deferred
    // (owed when the read came) or prefetched are remembered for the next step
    void note_use(int need, int owed) { forced |= need & (owed | prefetched); }

    // the six Prev* columns: the step's deferred move (no shift since), or the
    // copy a lazy shift left as views of the current ones
    template <class Ex> int settle_prev6(Ex &ex)
    {
        Half &c = half[tb];
        if (c.six_owed) {
            if (int rc = ex.move(kPartPrev6, c.six_lazy)) return rc;
            c.six_owed = false;
            return 0;
        }
        if (!c.prev_lazy) return 0;
        if (int rc = ex.shift(true)) return rc;
        c.prev_lazy = false;
        return 0;
    }

    // lazy HiddenState ends: the lazy half's PrevHiddenState gathered from the
    // base along the composed map into its storage -- the state a fused shift
    // leaves (HiddenState its view while h_alias holds), whichever half is
    // lazy, so every deferred move that follows finds real rows.  Never in
    // place: when the base is that storage the rows go to the other half's
    // PrevHiddenState storage and the halves exchange the two (that one is free
    // while the state holds: the other half's PrevHiddenState is dead after a
    // shift, and owed -- written before it is read -- after a step)
    template <class Ex> int end_hidden(Ex &ex)
    {
        if (!hid_lazy) return 0;
        const bool exchange = ph_store[hid_half] == hid_base;
        if (exchange) std::swap(ph_store[0], ph_store[1]);
        if (int rc = ex.gather_hidden(hid_half, hid_map, holder(hid_base), hid_word, exchange)) return rc;
        hid_lazy = false;
        return 0;
    }

    // owed PrevAction ends: the gather the shift did not launch, into the owed
    // half's PrevAction storage (a storage of the other half is the base: never
    // in place).  What is left is what the fused shift leaves: PrevAction real,
    // Action its view while a_alias holds (a whole-table writer has cleared it
    // otherwise)
    template <class Ex> int end_prev_action(Ex &ex)
    {
        if (!pa_lazy) return 0;
        if (int rc = ex.gather_prev_action(pa_half, pa_par, pa_base_prev)) return rc;
        pa_lazy = false;
        return 0;
    }

    // the deferred K4 part: PrevAction / PrevHiddenState of the current half from
    // the other half, along the last step's src_of (both intact until the next
    // step's K3a / K4)
    template <class Ex> int settle_prev_ah(Ex &ex)
    {
        Half &c = half[tb];
        if (!c.prev_ah_owed) return 0;
        if (int rc = end_hidden(ex)) return rc;        // (its source is the last half's PrevHiddenState)
        if (int rc = end_prev_action(ex)) return rc;   // (... and its PrevAction)
        // the Prev storage holds the current columns (aliased): copied out before
        // the Prev move overwrites it
        const int cols = (c.a_alias ? kAction : 0) | (c.h_alias ? kHidden : 0);
        if (cols)
            if (int rc = settle_cur_ah(ex, cols)) return rc;
        if (int rc = ex.move(kPartPrevAH, false)) return rc;
        c.prev_ah_owed = false;
        return 0;
    }

    // the deferred Action / HiddenState move of the current half (K1, the learner
    // and every accessor of the two columns need it; a shift fuses it); then the
    // columns of `out` a fused shift left as views of their Prev columns are
    // copied out
    template <class Ex> int settle_cur_ah(Ex &ex, int out)
    {
        Half &c = half[tb];
        // (lazy HiddenState: the move's source, or the column copied out)
        if (c.cur_ah_owed || ((out & kHidden) && c.h_alias))
            if (int rc = end_hidden(ex)) return rc;
        // (owed PrevAction: the move's source view, or -- its base -- the storage
        // the move writes; the column copied out; and whatever is owed by the
        // last half, whose storages the caller's writes reach next)
        if (pa_lazy && (c.cur_ah_owed || pa_half != tb || ((out & kAction) && c.a_alias)))
            if (int rc = end_prev_action(ex)) return rc;
        if (c.cur_ah_owed) {
            if (int rc = ex.move(kPartAH, false)) return rc;
            c.cur_ah_owed = false;
        }
        const bool ca = (out & kAction) && c.a_alias, ch = (out & kHidden) && c.h_alias;
        if (!ca && !ch) return 0;
        if (int rc = ex.copy_out(ca, ch)) return rc;
        if (ca) c.a_alias = false;
        if (ch) c.h_alias = false;
        return 0;
    }

    // the deferred prev-sensor move of the current half (accessors of the prev
    // sensor, construct_obs(prev), checkpoints; its source rows are the sensor's
    // before the last)
    template <class Ex> int settle_psem(Ex &ex)
    {
        Half &c = half[tb];
        if (!c.psem_owed) return 0;
        if (int rc = ex.wait_prev_sensor()) return rc;
        if (int rc = ex.move(kPartSensor, false)) return rc;
        c.psem_owed = false;
        return 0;
    }
};

}  // namespace defer
}  // namespace mbots
