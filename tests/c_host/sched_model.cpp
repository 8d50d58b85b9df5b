// The step's cross-queue ordering (csrc/mbots_sched.hpp) run over a symbolic
// executor: every launch of the manager's calls is an operation on a queue
// with a vector clock, every wait the schedule issues an edge, and every
// access of a buffer two queues share is checked against the accesses before
// it -- a read happens-after the last write, a write after every earlier read
// and write.  Stand-alone (tests/test_sched_model.py builds it with g++ and the
// address / undefined-behaviour sanitizers and runs it); no HIP, no GPU.
//
// Edges: an event wait, from the queue position at the event's last record; a
// value wait, from the store of the first epoch >= the waited one; the drain,
// from everything.  A wait inside a capture on an event recorded outside that
// capture gives no edge and is a finding.  Captured operations are not
// executed: they are kept, and a replay runs them as one unit on the stream of
// the manager's last call (the caller's side) and on a branch of its own (the
// sensor's side), after a drain -- a graph is launched on a quiet device --
// and the stream goes on after all of it.
//
// THE ACCESS TABLE (mbots_kernels.hpp SimState; DESIGN.md 2, the step's
// launches): what each launch of step t (buffers of parity p, table halves
// cur -> nxt) reads and writes of the buffers two queues share.
//
//   launch      queue    reads                            writes
//   reset pass  K1's     (the caller's reset flags)       State[p^1] (the half K1 reads)
//   K1          K1's     State[p^1], Act[cur], Lists[p^1] State[p], ObsrowOut[p]
//                        Finder (not in K1-finder mode)
//   K2          K1's     --                               RowBase[p] (row bases and the
//                                                         sensor order), Lists[p]
//   sensor      sensor's State[p], RowBase[p], Lists[p]   Finder, Sem[nxt]
//                        K1-finder: ObsrowOut[p],         K1-finder: PrevSem[nxt]
//                        Sem[cur]
//   K3a         caller's ObsrowOut[p], RowBase[p]         SrcOf[p]
//   prev-sensor caller's Sem[last half], SrcOf[last p]    PrevSem[cur]
//   move
//   sensor-row  caller's Sem[cur]                         --   (accessors, packers,
//   read                                                       construct_obs)
//   prev-sensor caller's PrevSem[cur]                     --
//   read
//   action      caller's --                               Act[cur]
//   write
#include "mbots_sched.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace mbots::sched;

namespace {

constexpr int kS0 = 0, kS1 = 1, kQS = 2, kQG = 3, kNQ = 4;   // two caller streams, the sensor's queue, a replay's sensor branch
using VC = std::array<int, kNQ>;
void join_into(VC &a, const VC &b)
{
    for (int i = 0; i < kNQ; ++i) a[i] = std::max(a[i], b[i]);
}

enum Buf { State0, State1, Finder, RowBase0, RowBase1, ObsrowOut0, ObsrowOut1, SrcOf0, SrcOf1, Lists0, Lists1,
           Sem0, Sem1, PrevSem0, PrevSem1, Act0, Act1, kNumBuf };
const char *const kBufName[kNumBuf] = {"State[0]", "State[1]", "Finder", "RowBase[0]", "RowBase[1]", "ObsrowOut[0]",
                                       "ObsrowOut[1]", "SrcOf[0]", "SrcOf[1]", "Lists[0]", "Lists[1]", "Sem[0]",
                                       "Sem[1]", "PrevSem[0]", "PrevSem[1]", "Act[0]", "Act[1]"};
struct Launch {
    const char *name;
    int n = 0;
    struct { int buf; bool write; } acc[10] = {};
    Launch(const char *nm = "") : name(nm) {}
    Launch &r(int b) { acc[n++] = {b, false}; return *this; }
    Launch &w(int b) { acc[n++] = {b, true}; return *this; }
};
struct Op {
    VC c{};
    int q = 0;
    const char *name = "";
};
bool before(const Op &a, const Op &b) { return a.c[a.q] <= b.c[a.q]; }

// the calls of a sequence
enum Call { kStep, kStepBehind, kShift, kShiftMove, kReadSem, kReadPrev, kWrite, kOther, kJoinCall, kIdle,
            kCapBegin, kCapEnd, kReplay, kNumCalls };
const char *const kCallName[kNumCalls] = {"step", "step(host behind)", "shift", "shift+prev-sensor move", "read sensor rows",
                                          "read prev-sensor rows", "write actions", "switch stream", "join", "idle reset",
                                          "begin capture", "end capture", "replay"};

struct Config {
    Mode mode;
    bool armed = false;
    // the model's own seeded faults
    bool single_obsrow = false;   // ObsrowOut single-buffered (the ADVICE r5 race)
    bool equality = false;        // value waits pass only on the exact epoch
    bool no_join = false;         // the round-5 probe: K1 does not wait for the last sensor
    uint32_t epoch_start = 0;
};

struct Finding {
    std::vector<int> seq;
    std::string detail;
};
std::map<std::string, Finding> g_findings;
const std::vector<int> *g_seq = nullptr;
void finding(const std::string &kind, const std::string &detail)
{
    auto it = g_findings.find(kind);
    if (it == g_findings.end() || g_seq->size() < it->second.seq.size()) g_findings[kind] = {*g_seq, detail};
}

struct GOp {
    enum { kLaunch, kRecord, kWait } type;
    bool sensor_side;
    int ev;
    Launch l;
};

struct Model {
    Config cfg;
    Schedule sched;
    // the device
    VC qc[kNQ]{};
    struct { bool has_w = false; Op w; std::vector<Op> reads; } buf[kNumBuf];
    struct { bool rec = false; VC c{}; } ev[kNumEvents];   // an event's last executed record
    unsigned long long ev_tag[kNumEvents] = {};            // the capture its last issued record belongs to
    struct Store { uint32_t v; Op op; };
    std::vector<Store> stores[2];
    struct EqWait { int sig; uint32_t v; Op op; };
    std::vector<EqWait> eq_waits;
    // the manager's side
    int tb = 0, par = 1;
    bool psem_owed = false;
    int stream = kS0;
    unsigned long long cap[2] = {0, 0}, next_cap = 0;
    std::vector<GOp> recording, graph;
    bool has_graph = false;
    std::vector<std::string> *log = nullptr;   // the executor's calls (the per-step edge table)

    Op run(int q, const Launch &l)
    {
        ++qc[q][q];
        Op op{qc[q], q, l.name};
        for (int i = 0; i < l.n; ++i) {
            auto &b = buf[l.acc[i].buf];
            const std::string what = std::string(l.name) + (l.acc[i].write ? " writes " : " reads ") + kBufName[l.acc[i].buf];
            if (b.has_w && !before(b.w, op)) finding("hazard: " + what + " beside " + b.w.name, "");
            if (l.acc[i].write) {
                for (const Op &rd : b.reads)
                    if (!before(rd, op)) finding("hazard: " + what + " beside " + rd.name, "");
                b.reads.clear();
                b.has_w = true;
                b.w = op;
            } else {
                b.reads.push_back(op);
            }
        }
        return op;
    }
    void store(int sig, uint32_t v, const Op &op)
    {
        for (const EqWait &w : eq_waits)
            if (w.sig == sig && v != w.v && !before(w.op, op))
                finding("hang: the equality wait for epoch " + std::string(sig == kFork ? "(fork)" : "(join)") +
                            " can be overtaken by the next store: it never passes", "");
        if (stores[sig].size() >= 4) stores[sig].erase(stores[sig].begin());
        stores[sig].push_back({v, op});
    }
    void drain()
    {
        VC all{};
        for (const VC &c : qc) join_into(all, c);
        for (VC &c : qc) c = all;
        eq_waits.clear();
    }
};

// the executor of one call on caller stream `s`
struct Exec {
    Model &m;
    int s;
    const char *call;
    unsigned long long in_cap() const { return m.cap[s]; }
    static const void *ptr(int stream) { return stream == kS0 ? nullptr : static_cast<const void *>(&kTag); }
    static int stream_of(const void *p) { return p == nullptr ? kS0 : kS1; }
    int queue(int q) const
    {
        switch (q) {
        case kSensor: return kQS;
        case kLast: return stream_of(m.sched.last_stream);
        case kCapture: return stream_of(m.sched.cap_stream);
        default: return s;
        }
    }
    const void *caller() const { return ptr(s); }
    int capture_of(int q, unsigned long long &id)
    {
        id = q == kSensor ? 0 : m.cap[queue(q)];
        return 0;
    }
    void note(const std::string &t)
    {
        if (m.log) m.log->push_back(t);
    }
    static const char *qname(int q) { return q == kSensor ? "sensor" : q == kLast ? "last" : "caller"; }
    static const char *ename(int e)
    {
        static const char *const n[] = {"join", "join", "totals", "caller-event", "hop"};
        return n[e];
    }
    int record(int e, int q)
    {
        note(std::string("record ") + ename(e) + " on " + qname(q));
        m.ev_tag[e] = in_cap();
        if (in_cap()) m.recording.push_back({GOp::kRecord, q == kSensor, e, {}});
        else m.ev[e] = {true, m.qc[queue(q)]};
        return 0;
    }
    int wait_event(int q, int e)
    {
        note(std::string("wait ") + qname(q) + " <- " + ename(e));
        if (in_cap()) {
            if (m.ev_tag[e] != in_cap())
                finding(std::string("capture: ") + call + " waits for an event recorded outside the capture", "");
            else
                m.recording.push_back({GOp::kWait, q == kSensor, e, {}});
            return 0;
        }
        if (m.cfg.no_join && q == kCaller && e <= kJoin1) return 0;
        if (m.ev[e].rec) join_into(m.qc[queue(q)], m.ev[e].c);
        return 0;
    }
    int wait_value(int q, int sig, uint32_t v)
    {
        note(std::string("wait ") + qname(q) + " <- " + (sig == kFork ? "fork" : "join") + " flag >= epoch");
        if (m.cfg.no_join && q == kCaller) return 0;
        const Model::Store *from = nullptr;
        for (const Model::Store &st : m.stores[sig])
            if (m.cfg.equality ? st.v == v : st.v >= v) {
                from = &st;
                break;
            }
        if (!from) {
            finding("hang: a value wait for an epoch nobody stores", call);
            return 0;
        }
        const int qi = queue(q);
        join_into(m.qc[qi], from->op.c);
        if (m.cfg.equality) {
            ++m.qc[qi][qi];
            m.eq_waits.push_back({sig, v, Op{m.qc[qi], qi, "wait"}});
        }
        return 0;
    }
    int raise_join(uint32_t v)
    {
        note("store join flag on sensor");
        m.store(kJoin, v, m.run(kQS, Launch{"the join flag's store"}));
        return 0;
    }
    bool pending(int) { return pending_answer; }
    int drain_and_zero()
    {
        note("drain");
        m.drain();
        m.stores[0].clear();
        m.stores[1].clear();
        return 0;
    }
    int refuse(Refusal, uint64_t) { return 1; }
    bool pending_answer = true;

    // a launch of the manager's, with the event its dispatch carries (-1: none)
    void launch(int q, const Launch &l, int rides = -1, uint32_t fork_epoch = 0)
    {
        if (in_cap()) {
            m.recording.push_back({GOp::kLaunch, q == kSensor, -1, l});
        } else {
            const Op op = m.run(queue(q), l);
            if (fork_epoch) m.store(kFork, fork_epoch, op);
        }
        if (rides >= 0) {
            m.ev_tag[rides] = in_cap();
            if (in_cap()) m.recording.push_back({GOp::kRecord, q == kSensor, rides, {}});
            else m.ev[rides] = {true, m.qc[queue(q)]};
        }
    }
    static const char kTag;
};
const char Exec::kTag = 0;

int state(int p) { return State0 + p; }

// mbots_step's launches in order, each after its call into the schedule
int do_step(Model &m, Exec &ex)
{
    Schedule &sc = m.sched;
    const bool k1f = sc.mode.k1_finder;
    Step sp;
    if (int rc = sc.begin_step(ex, sp)) return rc;
    const int p = m.par, cur = m.tb, nxt = m.tb ^ 1;
    const int obs = m.cfg.single_obsrow && k1f ? ObsrowOut0 : ObsrowOut0 + p;
    if (int rc = sc.before_k1(ex, sp)) return rc;
    if (m.cfg.armed) {
        if (int rc = sc.before_reset_pass(ex, sp)) return rc;
        ex.launch(sp.kq, Launch{"the reset pass"}.w(state(p ^ 1)));
    }
    Launch k1{"K1"};
    k1.r(state(p ^ 1)).r(Act0 + cur).r(Lists0 + (p ^ 1)).w(state(p)).w(obs);
    if (!k1f) k1.r(Finder);
    ex.launch(sp.kq, k1);
    if (int rc = sc.before_k2(ex, sp)) return rc;
    if (sp.k2_epoch) ex.note("store fork flag by K2");
    ex.launch(sp.kq, Launch{"K2"}.w(RowBase0 + p).w(Lists0 + p), kTotals, sp.k2_epoch);
    if (int rc = sc.before_sensor(ex, sp)) return rc;
    Launch sen{"the sensor"};
    sen.r(state(p)).r(RowBase0 + p).r(Lists0 + p).w(Finder).w(Sem0 + nxt);
    if (k1f) sen.r(obs).r(Sem0 + cur).w(PrevSem0 + nxt);
    ex.launch(kSensor, sen, sp.join);
    if (int rc = sc.after_sensor(ex, sp)) return rc;
    ex.launch(kCaller, Launch{"K3a"}.r(obs).r(RowBase0 + p).w(SrcOf0 + p));
    m.tb ^= 1;
    m.par ^= 1;
    m.psem_owed = !k1f;
    return 0;
}

void prev_sensor_move(Model &m, Exec &ex)
{
    ex.launch(kCaller, Launch{"the prev-sensor move"}.r(Sem0 + (m.tb ^ 1)).r(SrcOf0 + (m.par ^ 1)).w(PrevSem0 + m.tb));
    m.psem_owed = false;
}

void replay(Model &m)
{
    m.drain();
    const int L = Exec::stream_of(m.sched.last_stream);
    struct { bool rec = false; VC c{}; } ev[kNumEvents];
    const int own = m.qc[kQG][kQG];
    m.qc[kQG] = VC{};
    m.qc[kQG][kQG] = own;
    for (const GOp &g : m.graph) {
        const int q = g.sensor_side ? kQG : L;
        if (g.type == GOp::kLaunch) m.run(q, g.l);
        else if (g.type == GOp::kRecord) ev[g.ev] = {true, m.qc[q]};
        else if (ev[g.ev].rec) join_into(m.qc[q], ev[g.ev].c);
    }
    join_into(m.qc[L], m.qc[kQG]);
}

// one call of a sequence; false: it is no call in this state (the sequence is skipped)
bool apply(Model &m, int call)
{
    Exec ex{m, m.stream, kCallName[call]};
    Schedule &sc = m.sched;
    switch (call) {
    case kStep: case kStepBehind:
        if (call == kStepBehind && (!sc.mode.values() || m.cap[m.stream])) return false;   // (nobody asks)
        ex.pending_answer = call == kStep;
        do_step(m, ex);
        return true;
    case kShift: case kShiftMove:
        if (sc.enter(ex)) return true;
        if (call == kShiftMove) {
            if (!m.psem_owed && !sc.mode.k1_finder) return false;
            if (sc.wait_prev_sensor(ex)) return true;
            if (m.psem_owed) prev_sensor_move(m, ex);
        }
        return true;
    case kReadSem:
        if (sc.enter(ex) || sc.wait_sensor(ex)) return true;
        ex.launch(kCaller, Launch{"a sensor-row read"}.r(Sem0 + m.tb));
        return true;
    case kReadPrev:
        if (sc.enter(ex)) return true;
        if (m.psem_owed) {
            if (sc.wait_prev_sensor(ex)) return true;
            prev_sensor_move(m, ex);
        }
        if (sc.mode.k1_finder && sc.wait_sensor(ex)) return true;   // (the sensor moved them)
        ex.launch(kCaller, Launch{"a prev-sensor read"}.r(PrevSem0 + m.tb));
        return true;
    case kWrite:
        if (sc.enter(ex)) return true;
        ex.launch(kCaller, Launch{"the action write"}.w(Act0 + m.tb));
        return true;
    case kOther:
        if (m.cap[kS0] || m.cap[kS1]) return false;   // (the model captures on one stream)
        m.stream ^= 1;
        return true;
    case kJoinCall:
        sc.join(ex);
        return true;
    case kIdle: {
        // a restore (checkpoint load, growth): refused under capture, behind the guard
        if (m.cap[kS0] || m.cap[kS1]) return false;
        Exec last{m, Exec::stream_of(sc.last_stream), kCallName[call]};
        if (sc.guard(last, kCaller)) return true;
        m.drain();
        sc.idle_reset();
        m.tb = 0;
        m.par = 0;
        m.psem_owed = false;
        return true;
    }
    case kCapBegin:
        if (m.cap[kS0] || m.cap[kS1] || m.has_graph) return false;
        m.cap[m.stream] = ++m.next_cap;
        m.recording.clear();
        return true;
    case kCapEnd:
        if (!m.cap[m.stream]) return false;
        m.cap[m.stream] = 0;
        m.graph = m.recording;
        m.has_graph = true;
        return true;
    case kReplay:
        if (!m.has_graph || m.cap[kS0] || m.cap[kS1] || m.sched.poisoned || (m.sched.cap_steps & 1)) return false;
        replay(m);
        return true;
    }
    return false;
}

Model fresh(const Config &c)
{
    Model m;
    m.cfg = c;
    m.sched.mode = c.mode;
    m.sched.epoch = c.epoch_start;
    return m;
}

uint64_t g_count = 0;
void enumerate(const Model &m, std::vector<int> &seq, int depth)
{
    if (depth == 0) {
        ++g_count;
        return;
    }
    for (int c = 0; c < kNumCalls; ++c) {
        Model n = m;
        seq.push_back(c);
        if (apply(n, c)) enumerate(n, seq, depth - 1);
        seq.pop_back();
    }
}

std::string show(const std::vector<int> &seq)
{
    std::string s;
    for (int c : seq) s += (s.empty() ? "" : ", ") + std::string(kCallName[c]);
    return s;
}

const struct { const char *name; Mode mode; } kModes[4] = {
    {"forked, events", {false, false, false, false}},
    {"forked, values", {false, true, true, false}},
    {"K1-finder", {true, false, false, false}},
    {"swapped", {false, false, false, true}},
};

// every sequence of `depth` calls, from each starting point, in each mode, armed and not
uint64_t explore(Config base, int depth)
{
    static const std::vector<int> kStarts[] = {
        {},
        {kStep, kStep},
        {kStep, kStep, kCapBegin, kStep, kStep, kJoinCall, kCapEnd},
        {kStep, kStep, kJoinCall, kCapBegin, kStep, kStep, kJoinCall, kCapEnd, kReplay},
        {kStep, kCapBegin, kStep, kCapEnd},
    };
    g_count = 0;
    for (const auto &md : kModes)
        for (int armed = 0; armed < 2; ++armed)
            for (const auto &start : kStarts) {
                base.mode = md.mode;
                base.armed = armed != 0;
                Model m = fresh(base);
                std::vector<int> seq;
                g_seq = &seq;
                bool ok = true;
                for (int c : start) {
                    seq.push_back(c);
                    ok = ok && apply(m, c);
                }
                if (ok) enumerate(m, seq, depth);
            }
    return g_count;
}

int g_wrapped = 0;   // random runs that crossed the epoch wrap
uint64_t random_runs(Config base, int runs, int len)
{
    uint64_t x = 0x9E3779B97F4A7C15ull, calls = 0;
    auto next = [&] {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    base.epoch_start = kEpochWrap - 5;
    for (int r = 0; r < runs; ++r) {
        base.mode = kModes[r % 4].mode;
        base.armed = (r / 4) % 2 != 0;
        Model m = fresh(base);
        std::vector<int> seq;
        g_seq = &seq;
        for (int i = 0; i < len; ++i) {
            const int c = next() % 3 == 0 ? int(next() % kNumCalls) : (next() % 4 ? kStep : kStepBehind);
            seq.push_back(c);
            if (apply(m, c)) ++calls;
            else seq.pop_back();
        }
        if (m.sched.epoch_wraps) ++g_wrapped;
    }
    return calls;
}

// the executor's calls of one steady-state step (the fourth, host ahead)
std::string step_edges(const Mode &mode, bool armed)
{
    Config c;
    c.mode = mode;
    c.armed = armed;
    Model m = fresh(c);
    std::vector<int> seq;
    g_seq = &seq;
    for (int i = 0; i < 3; ++i) apply(m, kStep);
    apply(m, kShiftMove);   // (K1-finder: the shift's wait for the sensor before the last)
    std::vector<std::string> log;
    m.log = &log;
    apply(m, kStep);
    std::string s;
    for (const auto &l : log) s += (s.empty() ? "" : "; ") + l;
    return s.empty() ? "none" : s;
}

int expect_findings(const char *what, const std::vector<std::string> &kinds)
{
    int bad = 0;
    for (const auto &f : g_findings) {
        bool known = false;
        for (const auto &k : kinds) known = known || f.first == k;
        if (!known) {
            std::printf("FAIL (%s): unexpected finding: %s\n    after: %s\n", what, f.first.c_str(), show(f.second.seq).c_str());
            ++bad;
        }
    }
    for (const auto &k : kinds)
        if (!g_findings.count(k)) {
            std::printf("FAIL (%s): expected finding did not appear: %s\n", what, k.c_str());
            ++bad;
        }
    return bad;
}

}  // namespace

int main()
{
    int bad = 0;
    // the mode choice (mbots_create / mbots_grow_capacity)
    {
        const Knobs def, off{false, -1}, noswap{true, 0};
        auto bits = [](const Mode &m) { return (m.k1_finder ? 1 : 0) | (m.value_fork ? 2 : 0) | (m.value_join ? 4 : 0) | (m.swap ? 8 : 0); };
        const struct { uint64_t w; uint32_t cap; bool fm, jm; Knobs k; int want; } t[] = {
            {64, 128, true, true, def, 1},     {2048, 256, true, true, def, 1},  {2048, 512, true, true, def, 0},
            {2049, 128, true, true, def, 6},   {2304, 128, true, false, def, 2}, {2304, 128, false, false, def, 0},
            {8192, 128, true, true, def, 6},   {8192, 128, true, true, off, 0},  {8193, 128, true, true, def, 8},
            {8320, 128, true, true, noswap, 0}, {65536, 128, true, true, off, 8}, {8320, 128, false, false, Knobs{true, 1}, 8},
        };
        for (const auto &c : t)
            if (bits(choose(c.w, c.cap, c.fm, c.jm, c.k)) != c.want) {
                std::printf("FAIL: choose(%llu worlds, %u slots) = %d, expected %d\n", (unsigned long long)c.w, c.cap,
                            bits(choose(c.w, c.cap, c.fm, c.jm, c.k)), c.want);
                ++bad;
            }
    }
    // the per-step edge table (DESIGN.md 4 "Schedule")
    const char *const kEdges[4][2] = {
        {"wait caller <- join; wait sensor <- totals", nullptr},
        {"wait caller <- join flag >= epoch; store fork flag by K2; wait sensor <- fork flag >= epoch; store join flag on sensor", nullptr},
        {"wait sensor <- totals", "wait caller <- join; wait sensor <- totals"},
        {"record caller-event on caller; wait sensor <- caller-event; wait caller <- totals", nullptr},
    };
    for (int i = 0; i < 4; ++i)
        for (int armed = 0; armed < 2; ++armed) {
            const std::string got = step_edges(kModes[i].mode, armed != 0);
            const char *want = kEdges[i][armed] ? kEdges[i][armed] : kEdges[i][0];
            std::printf("edges %-15s %-8s %s\n", kModes[i].name, armed ? "armed" : "unarmed", got.c_str());
            if (got != want) {
                std::printf("FAIL: expected %s\n", want);
                ++bad;
            }
        }
    {
        // K1-finder with no shift between the steps: K1's own wait, for the sensor before the last
        Config c;
        c.mode = kModes[2].mode;
        Model m = fresh(c);
        std::vector<int> seq;
        g_seq = &seq;
        for (int i = 0; i < 3; ++i) apply(m, kStep);
        std::vector<std::string> log;
        m.log = &log;
        apply(m, kStep);
        if (log.size() != 2 || log[0] != "wait caller <- join") {
            std::printf("FAIL: K1-finder step without shift\n");
            ++bad;
        }
    }

    // the parent's rules: every call order
    g_findings.clear();
    const int kDepth = 4;
    const uint64_t n = explore(Config{}, kDepth);
    std::printf("depth %d: %llu sequences\n", kDepth, (unsigned long long)n);
    const uint64_t rc = random_runs(Config{}, 400, 60);
    std::printf("random: %llu calls, %d runs crossed the epoch wrap\n", (unsigned long long)rc, g_wrapped);
    if (g_wrapped < 50) {   // (100 of the 400 runs use value waits, and start 5 epochs short of the wrap)
        std::printf("FAIL: too few random runs crossed the epoch wrap\n");
        ++bad;
    }
    for (const auto &f : g_findings) std::printf("finding: %s\n    after: %s\n", f.first.c_str(), show(f.second.seq).c_str());
    // Known of the rules as they are, kept (a later fix): join() and wait_sensor
    // (the sensor-row readers; in K1-finder mode the prev-sensor readers too)
    // wait for the last join event without the same-capture test the step and
    // wait_prev_sensor apply
    bad += expect_findings("the rules", {
        "capture: join waits for an event recorded outside the capture",
        "capture: read sensor rows waits for an event recorded outside the capture",
        "capture: read prev-sensor rows waits for an event recorded outside the capture",
    });

    // the seeded faults: the model must see them
    {
        g_findings.clear();
        Config c;
        c.single_obsrow = true;
        explore(c, 3);
        const auto it = g_findings.find("hazard: K1 writes ObsrowOut[0] beside the sensor");
        if (it == g_findings.end()) {
            std::printf("FAIL: single-buffered ObsrowOut in K1-finder mode was not reported\n");
            ++bad;
        } else {
            std::printf("seeded single ObsrowOut: %s after: %s\n", it->first.c_str(), show(it->second.seq).c_str());
        }
    }
    {
        g_findings.clear();
        Config c;
        c.equality = true;
        explore(c, 3);
        bool hang = false;
        for (const auto &f : g_findings) hang = hang || f.first.rfind("hang:", 0) == 0;
        std::printf("seeded equality waits, joins kept: %s\n", hang ? "a hang" : "no hang (every store follows the wait before it)");
        g_findings.clear();
        c.no_join = true;
        explore(c, 3);
        const std::string k = "hang: the equality wait for epoch (fork) can be overtaken by the next store: it never passes";
        const auto it = g_findings.find(k);
        if (it == g_findings.end()) {
            std::printf("FAIL: equality waits without the join were not reported\n");
            ++bad;
        } else {
            std::printf("seeded equality waits, no join: %s after: %s\n", it->first.c_str(), show(it->second.seq).c_str());
        }
    }
    if (bad) return 1;
    std::printf("ok\n");
    return 0;
}
