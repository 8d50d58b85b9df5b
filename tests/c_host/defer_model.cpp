// Stand-alone model check of the manager's deferred-column rules
// (madrona-bots_amd/csrc/mbots_defer.hpp; built and run by
// tests/test_defer_model.py with the sanitizers on, never loaded into Python).
//
// The rules run over tiny symbolic tables: two table halves, the two
// PrevHiddenState storages, the src_of / map / row-count slots of the two step
// parities, columns of at most 8 rows whose cells are distinct integer tokens.
// The executor performs the overwrites the device performs (a step writes the
// other half's current columns and sensor rows and this parity's src_of, map
// and row counts, and moves nothing else; writers write the storages they
// write), and a storage the state says holds nothing is scribbled with poison.
// Beside it an eager table restates, for row movement only, what the CPU mode
// does: a step moves every column that travels with a row at once, a shift
// copies current to Prev, the prev sensor is the old row's sensor.  After every
// call the columns it exposes must equal the eager table's token for token,
// and after a require_all every column must.
//
// Every call sequence to a fixed depth runs from six starting points, for the
// four combinations of owed PrevAction on/off and prev-sensor-by-sensor, then
// a smaller pass with graph capture in the alphabet, then fixed-seed random
// sequences.  defer_model [depth] [capture depth] [random sequences]
#include "mbots_defer.hpp"

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mbots::defer;

namespace {

constexpr int R = 8;   // the most rows a table has
using Col = std::array<int, R>;

// the six current columns and the six shift-owned Prev* columns travel
// together: one token column each
struct Table {
    Col action, hidden, paction, phidden, cur6, prev6, sem, psem;
};

enum Op {
    kStep, kShift, kReadAction, kReadHidden, kReadPrevAction, kReadPrevHidden, kReadPrev6, kReadPrevSensor,
    kWriteAction, kWriteActionHidden, kWriteActionPart, kSetAction, kActMemoryless, kActNoWrite, kActSomeMemory,
    kConstructObsPrev, kPackSlim, kPackLearner, kSave, kResetWorlds, kLoad,
    kNumOps,
    kStepCapturing = kNumOps, kShiftCapturing,
    kNumOpsCapture,
};
const char *const kOpName[kNumOpsCapture] = {
    "step", "shift", "read Action", "read HiddenState", "read PrevAction", "read PrevHiddenState", "read Prev6",
    "read prev sensor", "write Action", "write Action+HiddenState", "write Action in part", "set_action",
    "act (memoryless)", "act (memoryless, no write)", "act (memory on some species)", "construct_obs(prev)",
    "pack_learner_slim", "pack_learner (require_all)", "save (require_all)", "reset_worlds", "load (reset)",
    "step while capturing", "shift while capturing"};

struct World {
    // the device
    Table T[2];
    int n[2] = {0, 0};   // rows of each half
    Col src_of[2], map[2];
    int words[5] = {0, 0, 0, 0, 0};   // K2's row counts [parity], [2 + parity]; the lazy shift's own [4]
    // the eager reference
    Table E;
    int en = 0;
    // the state under test and its inputs
    Deferred d;
    Env env;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    int token = 1, poison = -1000;
    int waits = 0;
};

std::vector<int> g_path;   // the calls of the sequence being run
const char *g_start = "";
int g_variant = 0;

[[noreturn]] void mismatch(const char *what, int row, int got, int want)
{
    printf("MISMATCH in %s row %d: the device has %d, the eager table %d\n  variant pa_on=%d psem_by_sensor=%d, "
           "start \"%s\", calls:",
           what, row, got, want, g_variant & 1, (g_variant >> 1) & 1, g_start);
    for (int op : g_path) printf(" [%s]", kOpName[op]);
    printf("\n");
    exit(1);
}
[[noreturn]] void broken(const char *what)
{
    printf("RULE BROKEN: %s\n  variant pa_on=%d psem_by_sensor=%d, start \"%s\", calls:", what, g_variant & 1,
           (g_variant >> 1) & 1, g_start);
    for (int op : g_path) printf(" [%s]", kOpName[op]);
    printf("\n");
    exit(1);
}

uint32_t rnd(World &w, uint32_t k)
{
    w.rng = w.rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(w.rng >> 33) % k;
}

// a half as its readers see it
struct View {
    const Col *action, *hidden;
};
View view(const World &w, int h)
{
    return {w.d.action_aliased(h) ? &w.T[h].paction : &w.T[h].action,
            w.d.hidden_aliased(h) ? &w.T[h].phidden : &w.T[h].hidden};
}
int at(const Col &c, int s) { return s < 0 ? 0 : c[(size_t)s]; }

// launch_move: the parts of `parts` from `src` (Action / HiddenState through
// `sv`) into `dst` along `map`
void do_move(const Table &src, View sv, Table &dst, int rows, const Col &map, int parts, bool six_lazy)
{
    for (int r = 0; r < rows; ++r) {
        const int s = map[(size_t)r];
        if (parts & kPartAH) {
            dst.action[(size_t)r] = at(*sv.action, s);
            dst.hidden[(size_t)r] = at(*sv.hidden, s);
        }
        if (parts & kPartSensor) dst.psem[(size_t)r] = at(src.sem, s);
        if (parts & kPartPrev6) dst.prev6[(size_t)r] = at(six_lazy ? src.cur6 : src.prev6, s);
        if (parts & kPartPrevAH) {
            dst.paction[(size_t)r] = at(src.paction, s);
            dst.phidden[(size_t)r] = at(src.phidden, s);
        }
    }
}

// the executor: what the manager's launches do to the tables
struct Exec {
    World &w;
    const Col &src() const { return w.src_of[w.d.src_par < 0 ? 0 : w.d.src_par]; }
    int move(int part, bool six_lazy)
    {
        const int tb = w.d.tb;
        do_move(w.T[tb ^ 1], view(w, tb ^ 1), w.T[tb], w.n[tb], src(), part, six_lazy);
        return 0;
    }
    int move_shift(int word)
    {
        const int tb = w.d.tb;
        const View sv = view(w, tb ^ 1);
        for (int r = 0; r < w.n[tb]; ++r) {
            const int s = src()[(size_t)r];
            w.T[tb].paction[(size_t)r] = at(*sv.action, s);
            if (word < 0) w.T[tb].phidden[(size_t)r] = at(*sv.hidden, s);
        }
        if (word >= 0) w.words[word] = w.n[tb];
        return 0;
    }
    int shift(bool rest)
    {
        Table &t = w.T[w.d.tb];
        if (rest) t.prev6 = t.cur6;
        else t.paction = t.action, t.phidden = t.hidden;
        return 0;
    }
    int gather_hidden(int half, int map, int base_half, int word, bool exchange)
    {
        if (exchange) std::swap(w.T[0].phidden, w.T[1].phidden);
        if (base_half == half) broken("the HiddenState gather runs in place");
        for (int r = 0; r < w.words[word]; ++r)
            w.T[half].phidden[(size_t)r] = at(w.T[base_half].phidden, w.map[map][(size_t)r]);
        w.words[word] = 0;
        return 0;
    }
    int gather_prev_action(int half, int par, bool base_prev)
    {
        const Table &b = w.T[half ^ 1];
        for (int r = 0; r < w.words[2 + par]; ++r)
            w.T[half].paction[(size_t)r] = at(base_prev ? b.paction : b.action, w.src_of[par][(size_t)r]);
        w.words[2 + par] = 0;
        return 0;
    }
    int copy_out(bool action, bool hidden)
    {
        Table &t = w.T[w.d.tb];
        if (action) t.action = t.paction;
        if (hidden) t.hidden = t.phidden;
        return 0;
    }
    int wait_prev_sensor()
    {
        ++w.waits;
        return 0;
    }
};

void fill(Col &c, int rows, int &token)
{
    for (int r = 0; r < R; ++r) c[(size_t)r] = r < rows ? token++ : 0;
}

// a storage the state says holds nothing is scribbled over -- but for the one
// a lazy column's base lives in (the rules keep it unwritten instead)
void scribble(World &w)
{
    const Deferred &d = w.d;
    auto blot = [&](Col &c) { for (int &v : c) v = w.poison--; };
    const Col *hid_base = d.hid_lazy ? &w.T[d.holder(d.hid_base)].phidden : nullptr;
    const Col *pa_base =
        d.pa_lazy ? (d.pa_base_prev ? &w.T[d.pa_half ^ 1].paction : &w.T[d.pa_half ^ 1].action) : nullptr;
    for (int h = 0; h < 2; ++h) {
        Table &t = w.T[h];
        const Half &f = d.half[h];
        const bool cur = h == d.tb;
        if ((f.a_alias || (cur && f.cur_ah_owed)) && &t.action != pa_base) blot(t.action);
        if (f.h_alias || (cur && f.cur_ah_owed)) blot(t.hidden);
        if (((cur && f.prev_ah_owed) || (d.pa_lazy && d.pa_half == h)) && &t.paction != pa_base) blot(t.paction);
        if (((cur && f.prev_ah_owed) || (d.hid_lazy && d.hid_half == h)) && &t.phidden != hid_base) blot(t.phidden);
        if ((cur && f.six_owed) || f.prev_lazy) blot(t.prev6);
        if (cur && f.psem_owed) blot(t.psem);
    }
}

void same(const char *what, const Col &dev, const Col &eager, int rows)
{
    for (int r = 0; r < rows; ++r)
        if (dev[(size_t)r] != eager[(size_t)r]) mismatch(what, r, dev[(size_t)r], eager[(size_t)r]);
}

// the six Prev* columns as construct_obs(prev) and the slim pack read them: the
// step's owed move gathered inside their own launch, or the lazy shift's view
void same_prev6(const World &w, const char *what)
{
    const Deferred &d = w.d;
    const Table &t = w.T[d.tb], &o = w.T[d.tb ^ 1];
    for (int r = 0; r < w.en; ++r) {
        int v;
        if (d.six_owed()) v = at(d.six_lazy() ? o.cur6 : o.prev6, w.src_of[d.src_par][(size_t)r]);
        else v = (d.prev_is_current() ? t.cur6 : t.prev6)[(size_t)r];
        if (v != w.E.prev6[(size_t)r]) mismatch(what, r, v, w.E.prev6[(size_t)r]);
    }
}

void same_all(const World &w)
{
    const Table &t = w.T[w.d.tb];
    same("Action", t.action, w.E.action, w.en);
    same("HiddenState", t.hidden, w.E.hidden, w.en);
    same("PrevAction", t.paction, w.E.paction, w.en);
    same("PrevHiddenState", t.phidden, w.E.phidden, w.en);
    same("the six current columns", t.cur6, w.E.cur6, w.en);
    same("the six Prev* columns", w.d.prev_is_current() ? t.cur6 : t.prev6, w.E.prev6, w.en);
    same("sensor", t.sem, w.E.sem, w.en);
    same("prev sensor", t.psem, w.E.psem, w.en);
}

void step(World &w, bool capturing)
{
    Exec ex{w};
    Deferred &d = w.d;
    w.env.capturing = capturing;
    if (capturing) w.env.graph_exists = true;   // (the manager notes the capture before anything else)
    StepPlan plan;
    if (d.begin_step(ex, w.env, plan)) broken("begin_step failed");
    const int tb = d.tb, nt = tb ^ 1, par = d.parity;
    // K1 reads the learner's actions through the view
    same("Action as K1 reads it", *view(w, tb).action, w.E.action, w.en);
    if (plan.map_out >= 0 && plan.map_out != par) broken("K3a writes another parity's map");
    if (plan.map_in == par) broken("K3a composes the map in place");
    // this step's src_of: births, deaths and reordering, another row count
    const int n_old = w.en, n_new = 3 + (int)rnd(w, R - 2);
    int perm[R];
    for (int r = 0; r < n_old; ++r) perm[r] = r;
    for (int r = n_old - 1; r > 0; --r) std::swap(perm[r], perm[rnd(w, (uint32_t)r + 1)]);
    Col src{};
    for (int r = 0, k = 0; r < R; ++r) src[(size_t)r] = r < n_new && k < n_old && rnd(w, 4) ? perm[k++] : -1;
    // the device: K3b's sensor rows (and in K1-finder mode the prev sensor), K3a's
    // current columns, src_of and map, K2's row counts, the prefetch move
    Table &nx = w.T[nt];
    Table e{};
    fill(e.cur6, n_new, w.token);
    fill(e.sem, n_new, w.token);
    nx.cur6 = e.cur6;
    nx.sem = e.sem;
    if (w.env.psem_by_sensor)
        for (int r = 0; r < n_new; ++r) nx.psem[(size_t)r] = at(w.T[tb].sem, src[(size_t)r]);
    if (plan.map_out >= 0)
        for (int r = 0; r < R; ++r) {
            const int s = src[(size_t)r];
            w.map[par][(size_t)r] = plan.map_in >= 0 && s >= 0 ? w.map[plan.map_in][(size_t)s] : s;
        }
    w.src_of[par] = src;
    if (plan.store_rows) w.words[par] = w.words[2 + par] = n_new;
    w.n[nt] = n_new;
    do_move(w.T[tb], view(w, tb), nx, n_new, src, plan.prefetch, plan.lazy != 0);
    d.end_step(plan, w.env.psem_by_sensor);
    // the eager table: every column that travels with a row moves at once
    for (int r = 0; r < n_new; ++r) {
        const int s = src[(size_t)r];
        e.action[(size_t)r] = at(w.E.action, s);
        e.hidden[(size_t)r] = at(w.E.hidden, s);
        e.paction[(size_t)r] = at(w.E.paction, s);
        e.phidden[(size_t)r] = at(w.E.phidden, s);
        e.prev6[(size_t)r] = at(w.E.prev6, s);
        e.psem[(size_t)r] = at(w.E.sem, s);
    }
    w.E = e;
    w.en = n_new;
    w.env.capturing = false;
    if (capturing && (d.hid_lazy || d.pa_lazy)) broken("a capturing step left a lazy state behind");
}

void write_rows(World &w, bool action, bool hidden, int first, int stride)
{
    Table &t = w.T[w.d.tb];
    for (int r = first; r < w.en; r += stride) {
        if (action) t.action[(size_t)r] = w.E.action[(size_t)r] = w.token++;
        if (hidden) t.hidden[(size_t)r] = w.E.hidden[(size_t)r] = w.token++;
    }
}

void call(World &w, int op)
{
    Exec ex{w};
    Deferred &d = w.d;
    const bool graph = w.env.graph_exists || op == kStepCapturing || op == kShiftCapturing;
    const bool was_hid = d.hid_lazy, was_pa = d.pa_lazy;
    int rc = 0;
    switch (op) {
    case kStep: step(w, false); break;
    case kStepCapturing: step(w, true); break;
    case kShift: case kShiftCapturing:
        w.env.capturing = op == kShiftCapturing;
        rc = d.shift(ex, w.env);
        w.env.capturing = false;
        w.E.paction = w.E.action;
        w.E.phidden = w.E.hidden;
        w.E.prev6 = w.E.cur6;
        break;
    case kReadAction:
        rc = d.require(ex, kAction, How::Rows);
        same("Action", w.T[d.tb].action, w.E.action, w.en);
        break;
    case kReadHidden:
        rc = d.require(ex, kHidden, How::Rows);
        same("HiddenState", w.T[d.tb].hidden, w.E.hidden, w.en);
        break;
    case kReadPrevAction:
        rc = d.require(ex, kPrevAction, How::Rows);
        same("PrevAction", w.T[d.tb].paction, w.E.paction, w.en);
        break;
    case kReadPrevHidden:
        rc = d.require(ex, kPrevHidden, How::Rows);
        same("PrevHiddenState", w.T[d.tb].phidden, w.E.phidden, w.en);
        break;
    case kReadPrev6:
        rc = d.require(ex, kPrev6, How::Rows);
        same("the six Prev* columns", w.T[d.tb].prev6, w.E.prev6, w.en);
        break;
    case kReadPrevSensor:
        rc = d.require(ex, kPrevSensor, How::Rows);
        same("prev sensor", w.T[d.tb].psem, w.E.psem, w.en);
        break;
    case kWriteAction:
        rc = d.require(ex, kAction, How::WriteAll);
        write_rows(w, true, false, 0, 1);
        break;
    case kWriteActionHidden:
        rc = d.require(ex, kAction | kHidden, How::WriteAll);
        write_rows(w, true, true, 0, 1);
        break;
    case kWriteActionPart:
        rc = d.require(ex, kAction, How::WritePart);
        write_rows(w, true, false, 0, 2);
        break;
    case kSetAction:
        rc = d.require(ex, kAction, How::Rows);
        write_rows(w, true, false, w.en - 1, R);
        break;
    case kActMemoryless:
        rc = d.require(ex, kAction, How::View);
        if (!rc) rc = d.require(ex, kAction, How::WriteAll);
        write_rows(w, true, false, 0, 1);
        break;
    case kActNoWrite: rc = d.require(ex, kAction, How::View); break;
    case kActSomeMemory:
        // the nets of some species read and write their rows' HiddenState; the
        // other rows keep theirs
        rc = d.require(ex, kAction | kHidden, How::View);
        same("HiddenState as the nets read it", *view(w, d.tb).hidden, w.E.hidden, w.en);
        if (!rc) rc = d.require(ex, kHidden, How::WritePart);
        if (!rc) rc = d.require(ex, kAction | kHidden, How::WriteAll);
        write_rows(w, true, false, 0, 1);
        write_rows(w, false, true, 1, 2);
        same("HiddenState after the act", w.T[d.tb].hidden, w.E.hidden, w.en);
        break;
    case kConstructObsPrev:
        // (the launch reads the six as they were owed before the sensor's move)
        same_prev6(w, "Prev6 as construct_obs(prev) reads it");
        rc = d.require(ex, kPrevSensor, How::Rows);
        same_prev6(w, "Prev6 as construct_obs(prev) reads it");
        same("prev sensor", w.T[d.tb].psem, w.E.psem, w.en);
        break;
    case kPackSlim:
        same_prev6(w, "Prev6 as the slim pack reads it");
        for (int r = 0; r < w.en; ++r) {
            const int v = d.psem_owed() ? at(w.T[d.tb ^ 1].sem, w.src_of[d.src_par][(size_t)r]) : w.T[d.tb].psem[(size_t)r];
            if (v != w.E.psem[(size_t)r]) mismatch("prev sensor as the slim pack reads it", r, v, w.E.psem[(size_t)r]);
        }
        break;
    case kPackLearner: case kSave:
        rc = d.require_all(ex, op == kPackLearner);
        same_all(w);
        break;
    case kResetWorlds:
        rc = d.require_prev_action_storage(ex);
        if (d.pa_lazy) broken("reset_worlds left PrevAction owed");
        break;
    case kLoad: {
        // a checkpoint load: the restored table is half 0, nothing is deferred
        const Table e = w.E;
        d.reset();
        w.T[0] = e;
        w.n[0] = w.en;
        break;
    }
    default: break;
    }
    if (rc) broken("a rule returned an error");
    if (graph && ((!was_hid && d.hid_lazy) || (!was_pa && d.pa_lazy)))
        broken("a lazy state was entered while capturing or with a graph");
    // the columns nobody defers are always there
    same("the six current columns", w.T[d.tb].cur6, w.E.cur6, w.en);
    same("sensor", w.T[d.tb].sem, w.E.sem, w.en);
    scribble(w);
}

// the end of every sequence: everything made real must be the eager table
void finish(const World &at_end)
{
    World w = at_end;
    Exec ex{w};
    if (w.d.require_all(ex, false)) broken("require_all failed");
    same_all(w);
}

World fresh(int variant)
{
    World w;
    w.env.pa_on = (variant & 1) != 0;
    w.env.psem_by_sensor = (variant & 2) != 0;
    w.en = w.n[0] = 6;
    Table &t = w.T[0];
    for (Col *c : {&t.action, &t.hidden, &t.paction, &t.phidden, &t.cur6, &t.prev6, &t.sem, &t.psem})
        fill(*c, w.en, w.token);
    w.E = t;
    for (Col *c : {&w.src_of[0], &w.src_of[1], &w.map[0], &w.map[1]}) c->fill(-1);
    scribble(w);
    return w;
}

struct Start {
    const char *name;
    int rounds;       // (step, shift, whole Action write) rounds
    bool last_write;  // the last round has its write
};
const Start kStarts[] = {{"fresh", 0, true},
                         {"one round", 1, true},
                         {"two rounds (lazy HiddenState entered)", 2, true},
                         {"three rounds (PrevAction owed too)", 3, true},
                         {"two rounds, the last without its write", 2, false},
                         {"three rounds, the last without its write", 3, false}};

World start_world(int variant, const Start &s)
{
    World w = fresh(variant);
    g_path.clear();
    for (int k = 0; k < s.rounds; ++k) {
        for (int op : {(int)kStep, (int)kShift, (int)kWriteAction}) {
            if (op == kWriteAction && k + 1 == s.rounds && !s.last_write) break;
            g_path.push_back(op);
            call(w, op);
        }
    }
    // the starting point is in the state named
    const Deferred &d = w.d;
    const bool ok = s.rounds == 0   ? !d.hid_lazy && !d.pa_lazy && !d.cur().h_alias
                    : s.rounds == 1 ? !d.hid_lazy && !d.pa_lazy && d.cur().h_alias
                    : s.rounds == 2 ? d.hid_lazy && d.hid_half == d.tb
                                    : d.hid_lazy && d.hid_half == d.tb && d.pa_lazy == w.env.pa_on;
    if (!ok || d.cur().a_alias != (s.rounds > 0 && !s.last_write)) broken("a starting point is not in the state named");
    return w;
}

uint64_t g_sequences = 0;

void explore(const World &w, int depth, int ops)
{
    if (depth == 0) {
        ++g_sequences;
        finish(w);
        return;
    }
    for (int op = 0; op < ops; ++op) {
        World next = w;
        g_path.push_back(op);
        call(next, op);
        explore(next, depth - 1, ops);
        g_path.pop_back();
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int depth = argc > 1 ? atoi(argv[1]) : 4;
    const int cap_depth = argc > 2 ? atoi(argv[2]) : 3;
    const int randoms = argc > 3 ? atoi(argv[3]) : 3000;
    for (g_variant = 0; g_variant < 4; ++g_variant)
        for (const Start &s : kStarts) {
            g_start = s.name;
            const World w = start_world(g_variant, s);
            const size_t base = g_path.size();
            explore(w, depth, kNumOps);
            g_path.resize(base);
        }
    const uint64_t plain = g_sequences;
    for (g_variant = 0; g_variant < 4; ++g_variant)
        for (const Start &s : kStarts) {
            g_start = s.name;
            const World w = start_world(g_variant, s);
            explore(w, cap_depth, kNumOpsCapture);
        }
    const uint64_t captured = g_sequences - plain;
    for (g_variant = 0; g_variant < 4; ++g_variant) {
        g_start = "fresh (random)";
        for (int k = 0; k < randoms; ++k) {
            World w = fresh(g_variant);
            w.rng += (uint64_t)k * 0x2545F4914F6CDD1Dull;
            g_path.clear();
            for (int c = 0; c < 40; ++c) {
                // (steps and shifts as often as everything else together)
                const uint32_t pick = rnd(w, 2 * kNumOps);
                const int op = pick < (uint32_t)kNumOps ? (int)pick : (pick & 1 ? kStep : kShift);
                g_path.push_back(op);
                call(w, op);
            }
            finish(w);
        }
    }
    printf("defer_model: depth %d: %llu sequences; with capture depth %d: %llu sequences; random: %d sequences of 40 "
           "calls; all equal to the eager table\n",
           depth, (unsigned long long)plain, cap_depth, (unsigned long long)captured, 4 * randoms);
    return 0;
}
