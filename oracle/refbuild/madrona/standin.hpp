/*
 * standin.hpp -- TEST INFRASTRUCTURE ONLY.
 *
 * A small single-threaded stand-in for the slice of the Madrona engine API that
 * the reference's simulation sources (sim.cpp, sim.hpp, sim.inl, types.hpp) use,
 * so that those sources compile and run without the engine.  It is written from
 * how those files use the API and from DESIGN.md section 3; it shares no code
 * with oracle/mbots_oracle.c or csrc/.  Wherever the engine, not the simulation
 * source, decides an outcome, this file implements DESIGN.md section 3:
 *
 *   - one host thread; ParallelForNode visits tables in registration order and
 *     rows in table order, skipping destroyed rows; rows created while a node
 *     runs are appended and not visited by that node
 *   - destroyEntity marks a row; the row stays readable until its table is next
 *     sorted (SortArchetypeNode) or until RecycleEntitiesNode, which compact
 *   - SortArchetypeNode<A, WorldID> is a stable sort by world;
 *     SortArchetypeNode<A, C> a stable sort by (first 32-bit word of C, world)
 *   - new rows are zero, tables never move in memory
 *   - Threefry-2x32-20 counter RNG, quaternion expressions as documented there
 */
#pragma once

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <initializer_list>
#include <numeric>
#include <type_traits>
#include <vector>

namespace madrona {

/* ---------------------------------------------------------------- basics */
struct Entity {
    uint32_t gen;
    int32_t id;
    static constexpr Entity none() { return Entity{0xFFFFFFFFu, -1}; }
};
inline bool operator==(Entity a, Entity b) { return a.gen == b.gen && a.id == b.id; }
inline bool operator!=(Entity a, Entity b) { return !(a == b); }

struct Loc {
    uint32_t archetype;
    int32_t row;
};

struct WorldID {
    int32_t idx;
};

template <typename... ComponentTs> struct Archetype {};

template <typename T> class Span {
public:
    Span() : ptr_(nullptr), n_(0) {}
    Span(T *p, size_t n) : ptr_(p), n_(n) {}
    Span(std::initializer_list<std::remove_const_t<T>> l) : ptr_(l.begin()), n_(l.size()) {}
    T *data() const { return ptr_; }
    size_t size() const { return n_; }
private:
    T *ptr_;
    size_t n_;
};

/* ---------------------------------------------------------------- atomics */
namespace sync {
enum class memory_order { relaxed, acquire, release, acq_rel, seq_cst };
}

/* One thread runs everything, so these are plain loads and stores. */
template <typename T> class AtomicT {
public:
    AtomicT() = default;
    AtomicT(T v) : v_(v) {}
    T load_relaxed() const { return v_; }
    void store_relaxed(T v) { v_ = v; }
    T fetch_add_relaxed(T v) { T o = v_; v_ = (T)(v_ + v); return o; }
    template <sync::memory_order, sync::memory_order>
    bool compare_exchange_weak(T &expected, T desired)
    {
        if (v_ == expected) { v_ = desired; return true; }
        expected = v_;
        return false;
    }
private:
    T v_;
};
using AtomicU32 = AtomicT<uint32_t>;
using AtomicI32 = AtomicT<int32_t>;

/* ---------------------------------------------------------------- math */
namespace math {

inline constexpr float pi = 3.14159265358979323846f;

struct Vector2 {
    float x, y;
    Vector2 &operator-=(const Vector2 &o) { x = x - o.x; y = y - o.y; return *this; }
    Vector2 &operator+=(const Vector2 &o) { x = x + o.x; y = y + o.y; return *this; }
};
inline Vector2 operator/(const Vector2 &a, float b) { return Vector2{a.x / b, a.y / b}; }
inline Vector2 operator*(const Vector2 &a, float b) { return Vector2{a.x * b, a.y * b}; }
inline Vector2 operator-(const Vector2 &a, const Vector2 &b) { return Vector2{a.x - b.x, a.y - b.y}; }
inline Vector2 operator+(const Vector2 &a, const Vector2 &b) { return Vector2{a.x + b.x, a.y + b.y}; }

struct Vector3 {
    float x, y, z;
    Vector3 &operator+=(const Vector3 &o) { x = x + o.x; y = y + o.y; z = z + o.z; return *this; }
    Vector3 &operator-=(const Vector3 &o) { x = x - o.x; y = y - o.y; z = z - o.z; return *this; }
    float length2() const { return x * x + y * y + z * z; }
    float length() const { return sqrtf(length2()); }
    /* sqrtf and one division per component */
    Vector3 normalize() const
    {
        float l = length();
        return Vector3{x / l, y / l, z / l};
    }
    Vector2 xy() const { return Vector2{x, y}; }
};
inline Vector3 operator+(const Vector3 &a, const Vector3 &b) { return Vector3{a.x + b.x, a.y + b.y, a.z + b.z}; }
inline Vector3 operator-(const Vector3 &a, const Vector3 &b) { return Vector3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline Vector3 operator*(const Vector3 &a, float b) { return Vector3{a.x * b, a.y * b, a.z * b}; }
inline Vector3 operator*(float b, const Vector3 &a) { return Vector3{b * a.x, b * a.y, b * a.z}; }
inline Vector3 operator/(const Vector3 &a, float b) { return Vector3{a.x / b, a.y / b, a.z / b}; }
inline Vector3 cross(const Vector3 &a, const Vector3 &b)
{
    return Vector3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

struct Diag3x3 {
    float d0, d1, d2;
};

struct Quat {
    float w, x, y, z;

    /* (cos a/2, axis sin a/2), the half-angle functions correctly rounded to
     * float (evaluated in double, rounded once) */
    static Quat angleAxis(float angle, Vector3 axis)
    {
        double h = (double)angle * 0.5;
        float c = (float)std::cos(h), s = (float)std::sin(h);
        return Quat{c, axis.x * s, axis.y * s, axis.z * s};
    }

    /* v + 2 (w (q x v) + q x (q x v)), q the vector part */
    Vector3 rotateVec(Vector3 v) const
    {
        Vector3 pure{x, y, z};
        Vector3 pv = cross(pure, v);
        Vector3 ppv = cross(pure, pv);
        return v + 2.0f * ((pv * w) + ppv);
    }

    Quat &operator*=(const Quat &o) { *this = mul(*this, o); return *this; }

    /* Hamilton product */
    static Quat mul(const Quat &a, const Quat &b)
    {
        return Quat{
            a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
            a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
            a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x,
        };
    }
};
inline Quat operator*(const Quat &a, const Quat &b) { return Quat::mul(a, b); }

}  // namespace math

/* ---------------------------------------------------------------- RNG */
struct RandKey {
    uint32_t a, b;
};

namespace rand {

inline uint32_t rotl(uint32_t v, unsigned r) { return (v << r) | (v >> (32u - r)); }

/* Threefry-2x32, 20 rounds (Salmon et al., "Parallel random numbers: as easy
 * as 1, 2, 3", SC11): five groups of four rounds, a key injection after each. */
inline RandKey threefry(RandKey key, uint32_t c0, uint32_t c1)
{
    const uint32_t ks[3] = {key.a, key.b, 0x1BD11BDAu ^ key.a ^ key.b};
    const unsigned rot[8] = {13, 15, 26, 6, 17, 29, 16, 24};
    uint32_t x = c0 + ks[0], y = c1 + ks[1];
    for (unsigned g = 0; g < 5; ++g) {
        for (unsigned r = 0; r < 4; ++r) {
            x += y;
            y = rotl(y, rot[(g & 1u) * 4u + r]) ^ x;
        }
        x += ks[(g + 1u) % 3u];
        y += ks[(g + 2u) % 3u] + (g + 1u);
    }
    return RandKey{x, y};
}

inline RandKey initKey(uint32_t seed) { return RandKey{seed, 0u}; }
inline RandKey split_i(RandKey key, uint32_t i, uint32_t j = 0) { return threefry(key, i, j); }
inline uint32_t bits32(RandKey key, uint32_t counter) { return threefry(key, counter, 0u).a; }
inline float bitsToFloat01(uint32_t bits) { return (float)(bits >> 8) * (1.0f / 16777216.0f); }

}  // namespace rand

class RNG {
public:
    RNG() : key_{0, 0}, ctr_(0) {}
    RNG(RandKey k) : key_(k), ctr_(0) {}
    uint32_t sampleBits() { return rand::bits32(key_, ctr_++); }
    float sampleUniform() { return rand::bitsToFloat01(sampleBits()); }
    int32_t sampleI32(int32_t a, int32_t b)
    {
        uint64_t range = (uint32_t)(b - a);
        return a + (int32_t)(((uint64_t)sampleBits() * range) >> 32);
    }
    RandKey key() const { return key_; }
    uint32_t counter() const { return ctr_; }
private:
    RandKey key_;
    uint32_t ctr_;
};

/* ---------------------------------------------------------------- ECS */
namespace detail {
inline uint32_t nextTypeID()
{
    static uint32_t n = 0;
    return n++;
}
}  // namespace detail

template <typename T> struct TypeTag {
    static uint32_t id()
    {
        static uint32_t v = detail::nextTypeID();
        return v;
    }
};

struct Table {
    std::vector<uint32_t> comps;   /* type ids; [0] Entity, [1] WorldID */
    std::vector<size_t> sizes;
    std::vector<char *> cols;      /* each maxRows + 1 rows, never moved */
    int32_t numRows = 0;
    std::vector<int32_t> worldOffsets, worldCounts;
    bool perEntity = true;         /* false: plain buffers (no Entity rows) */

    int find(uint32_t tid) const
    {
        for (size_t i = 0; i < comps.size(); ++i)
            if (comps[i] == tid) return (int)i;
        return -1;
    }
};

class StateManager {
public:
    struct Slot {
        uint32_t arch;
        int32_t row;   /* -1: gone */
    };

    explicit StateManager(uint32_t num_worlds, int32_t max_rows)
        : numWorlds(num_worlds), maxRows(max_rows), worldData(num_worlds, nullptr) {}

    ~StateManager()
    {
        for (Table &t : tables)
            for (char *c : t.cols) free(c);
    }

    StateManager(const StateManager &) = delete;
    StateManager &operator=(const StateManager &) = delete;

    template <typename ArchetypeT> uint32_t archID() const
    {
        uint32_t tid = TypeTag<ArchetypeT>::id();
        for (size_t i = 0; i < archTypes.size(); ++i)
            if (archTypes[i] == tid) return (uint32_t)i;
        fprintf(stderr, "stand-in: archetype not registered\n");
        abort();
    }

    template <typename ArchetypeT, typename... Cs> void addArchetype(Archetype<Cs...> *, bool per_entity = true)
    {
        uint32_t tid = TypeTag<ArchetypeT>::id();
        for (uint32_t t : archTypes)
            if (t == tid) return;
        static_assert((std::is_trivially_copyable_v<Cs> && ...), "components are moved with memcpy");
        Table t;
        t.perEntity = per_entity;
        t.comps = {TypeTag<Entity>::id(), TypeTag<WorldID>::id(), TypeTag<Cs>::id()...};
        t.sizes = {sizeof(Entity), sizeof(WorldID), sizeof(Cs)...};
        for (size_t s : t.sizes) {
            char *p = (char *)calloc((size_t)maxRows + 1, s);   /* + 1: padding row, stays zero */
            if (!p) abort();
            t.cols.push_back(p);
        }
        t.worldOffsets.assign(numWorlds, 0);
        t.worldCounts.assign(numWorlds, 0);
        archTypes.push_back(tid);
        tables.push_back(std::move(t));
    }

    template <typename ArchetypeT, typename ComponentT> ComponentT *getArchetypeComponent()
    {
        Table &t = tables[archID<ArchetypeT>()];
        int c = t.find(TypeTag<ComponentT>::id());
        if (c < 0) { fprintf(stderr, "stand-in: component not in archetype\n"); abort(); }
        return (ComponentT *)t.cols[(size_t)c];
    }
    template <typename ArchetypeT> uint32_t getArchetypeNumRows() { return (uint32_t)tables[archID<ArchetypeT>()].numRows; }
    template <typename ArchetypeT> int32_t *getArchetypeWorldOffsets() { return tables[archID<ArchetypeT>()].worldOffsets.data(); }
    template <typename ArchetypeT> int32_t *getArchetypeWorldCounts() { return tables[archID<ArchetypeT>()].worldCounts.data(); }

    /* n zeroed contiguous rows of one world at the end of the table */
    Loc addRows(uint32_t arch, int32_t world, int32_t n, Entity *first = nullptr)
    {
        Table &t = tables[arch];
        if (t.numRows + n > maxRows) {
            fprintf(stderr, "stand-in: table %u is full (%d rows)\n", arch, maxRows);
            abort();
        }
        int32_t row = t.numRows;
        for (size_t c = 0; c < t.cols.size(); ++c) memset(t.cols[c] + (size_t)row * t.sizes[c], 0, (size_t)n * t.sizes[c]);
        for (int32_t i = 0; i < n; ++i) {
            Entity e{0u, (int32_t)slots.size()};
            slots.push_back(Slot{arch, row + i});
            ((Entity *)t.cols[0])[row + i] = e;
            ((WorldID *)t.cols[1])[row + i] = WorldID{world};
            if (i == 0 && first) *first = e;
        }
        t.numRows += n;
        return Loc{arch, row};
    }

    Loc loc(Entity e) const
    {
        if (e.id < 0 || (size_t)e.id >= slots.size() || slots[(size_t)e.id].row < 0) {
            fprintf(stderr, "stand-in: use of a dead or invalid entity %d\n", e.id);
            abort();
        }
        return Loc{slots[(size_t)e.id].arch, slots[(size_t)e.id].row};
    }
    bool valid(Entity e) const { return e.id >= 0 && (size_t)e.id < slots.size() && slots[(size_t)e.id].row >= 0; }

    void *component(Loc l, uint32_t tid)
    {
        Table &t = tables[l.archetype];
        int c = t.find(tid);
        if (c < 0) { fprintf(stderr, "stand-in: component %u not in archetype %u\n", tid, l.archetype); abort(); }
        return t.cols[(size_t)c] + (size_t)l.row * t.sizes[(size_t)c];
    }

    /* deferred: the row keeps its data and its entity until the next compaction */
    void destroy(Entity e)
    {
        Loc l = loc(e);
        ((WorldID *)tables[l.archetype].cols[1])[l.row].idx = -1;
    }
    bool rowLive(uint32_t arch, int32_t row) const { return ((const WorldID *)tables[arch].cols[1])[row].idx >= 0; }

    /* Drop destroyed rows and reorder the rest by key (stable); keyed == false
     * keeps the order.  World offsets and counts follow the new order. */
    void rebuild(uint32_t arch, bool keyed, const std::function<uint64_t(int32_t)> &key)
    {
        Table &t = tables[arch];
        std::vector<int32_t> order;
        const WorldID *wid = (const WorldID *)t.cols[1];
        for (int32_t r = 0; r < t.numRows; ++r) {
            if (wid[r].idx >= 0) order.push_back(r);
            else slots[(size_t)((Entity *)t.cols[0])[r].id].row = -1;
        }
        if (keyed) {
            std::vector<uint64_t> k((size_t)t.numRows);
            for (int32_t r : order) k[(size_t)r] = key(r);
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return k[(size_t)a] < k[(size_t)b]; });
        }
        for (size_t c = 0; c < t.cols.size(); ++c) {
            size_t sz = t.sizes[c];
            std::vector<char> tmp(order.size() * sz);
            for (size_t i = 0; i < order.size(); ++i) memcpy(tmp.data() + i * sz, t.cols[c] + (size_t)order[i] * sz, sz);
            memcpy(t.cols[c], tmp.data(), tmp.size());
            memset(t.cols[c] + tmp.size(), 0, ((size_t)t.numRows - order.size()) * sz);
        }
        t.numRows = (int32_t)order.size();
        std::fill(t.worldCounts.begin(), t.worldCounts.end(), 0);
        for (int32_t r = 0; r < t.numRows; ++r) {
            slots[(size_t)((Entity *)t.cols[0])[r].id].row = r;
            t.worldCounts[(size_t)((WorldID *)t.cols[1])[r].idx] += 1;
        }
        int32_t off = 0;
        for (uint32_t w = 0; w < numWorlds; ++w) { t.worldOffsets[w] = off; off += t.worldCounts[w]; }
    }

    uint32_t numWorlds;
    int32_t maxRows;
    std::vector<uint32_t> archTypes;
    std::vector<Table> tables;
    std::vector<Slot> slots;
    std::vector<void *> worldData;
    /* run before an archetype's rows are compacted (the driver's B.4 hook) */
    std::function<void(uint32_t arch)> beforeCompact;
};

namespace mwGPU {
inline StateManager *&currentStateManager()
{
    static StateManager *p = nullptr;
    return p;
}
inline StateManager *getStateManager() { return currentStateManager(); }
}  // namespace mwGPU

class ECSRegistry {
public:
    explicit ECSRegistry(StateManager *sm) : sm_(sm) {}
    template <typename T> void registerComponent() {}
    template <typename T> void registerSingleton()
    {
        sm_->addArchetype<SingletonArchetype<T>>((Archetype<T> *)nullptr);
        singletons.push_back(sm_->archID<SingletonArchetype<T>>());
    }
    template <typename ArchetypeT> void registerArchetype() { sm_->addArchetype<ArchetypeT>((ArchetypeT *)nullptr); }
    template <typename ArchetypeT, typename ComponentT> void exportColumn(uint32_t slot)
    {
        if (exports.size() <= slot) exports.resize(slot + 1, {-1, 0u});
        exports[slot] = {(int32_t)sm_->archID<ArchetypeT>(), TypeTag<ComponentT>::id()};
    }
    template <typename T> void exportSingleton(uint32_t slot) { exportColumn<SingletonArchetype<T>, T>(slot); }

    template <typename T> struct SingletonArchetype : Archetype<T> {};
    struct Export {
        int32_t arch;
        uint32_t comp;
    };
    std::vector<Export> exports;
    std::vector<uint32_t> singletons;
    StateManager *stateManager() { return sm_; }
private:
    StateManager *sm_;
};

/* ---------------------------------------------------------------- context */
class Context {
public:
    Context(StateManager *sm, void *data, WorldID w) : sm_(sm), data_(data), world_(w) {}

    template <typename T> T &get(Entity e) { return *(T *)sm_->component(sm_->loc(e), TypeTag<T>::id()); }
    template <typename T> T &get(Loc l) { return *(T *)sm_->component(l, TypeTag<T>::id()); }
    template <typename ArchetypeT> Entity makeEntity()
    {
        Entity e;
        sm_->addRows(sm_->archID<ArchetypeT>(), world_.idx, 1, &e);
        return e;
    }
    template <typename ArchetypeT> Loc makeStationary(uint32_t n) { return sm_->addRows(sm_->archID<ArchetypeT>(), world_.idx, (int32_t)n); }
    void destroyEntity(Entity e) { sm_->destroy(e); }
    Loc loc(Entity e) const { return sm_->loc(e); }
    WorldID worldID() const { return world_; }
    StateManager *stateManager() { return sm_; }
    void *userData() const { return data_; }
private:
    StateManager *sm_;
    void *data_;
    WorldID world_;
};

template <typename ContextT, typename DataT> class CustomContext : public Context {
public:
    using Context::Context;
    DataT &data() const { return *(DataT *)userData(); }
};

struct WorldBase {
    explicit WorldBase(Context &) {}
};

/* ---------------------------------------------------------------- base components */
namespace base {
struct Position : math::Vector3 {
    Position() = default;
    Position(const math::Vector3 &v) : math::Vector3(v) {}
};
struct Rotation : math::Quat {
    Rotation() = default;
    Rotation(const math::Quat &q) : math::Quat(q) {}
};
struct Scale : math::Diag3x3 {
    Scale() = default;
    Scale(const math::Diag3x3 &d) : math::Diag3x3(d) {}
};
struct ObjectID {
    int32_t idx;
    int32_t aux;
};
inline void registerTypes(ECSRegistry &) {}
}  // namespace base

/* ---------------------------------------------------------------- task graphs */
class TaskGraph {
public:
    struct NodeID {
        uint32_t id;
    };

    class Builder {
    public:
        template <typename NodeT> NodeID addToGraph(Span<const NodeID> deps)
        {
            /* one thread: the order the nodes are added in is a valid order of the
             * graph as long as every dependency names an earlier node */
            for (size_t i = 0; i < deps.size(); ++i) assert(deps.data()[i].id < nodes.size());
            nodes.push_back(&NodeT::run);
            return NodeID{(uint32_t)nodes.size() - 1u};
        }
        std::vector<void (*)(StateManager &)> nodes;
    };
};
using TaskGraphBuilder = TaskGraph::Builder;

class TaskGraphManager {
public:
    template <typename EnumT> TaskGraph::Builder &init(EnumT id)
    {
        size_t i = (size_t)id;
        if (graphs.size() <= i) graphs.resize(i + 1);
        return graphs[i];
    }
    template <typename EnumT> void run(EnumT id, StateManager &sm)
    {
        mwGPU::currentStateManager() = &sm;
        for (auto fn : graphs[(size_t)id].nodes) fn(sm);
    }
    std::vector<TaskGraph::Builder> graphs;
};

template <typename ContextT, auto Fn, typename... ComponentTs> struct ParallelForNode {
    static void run(StateManager &sm)
    {
        const uint32_t ids[] = {TypeTag<ComponentTs>::id()...};
        for (uint32_t a = 0; a < sm.tables.size(); ++a) {
            Table &t = sm.tables[a];
            if (!t.perEntity) continue;
            bool all = true;
            for (uint32_t id : ids) all = all && t.find(id) >= 0;
            if (!all) continue;
            const int32_t n = t.numRows;   /* rows appended meanwhile are not visited */
            for (int32_t r = 0; r < n; ++r) {
                int32_t w = ((WorldID *)t.cols[1])[r].idx;
                if (w < 0) continue;
                ContextT ctx(&sm, sm.worldData[(size_t)w], WorldID{w});
                Fn(ctx, *(ComponentTs *)(t.cols[(size_t)t.find(TypeTag<ComponentTs>::id())] + (size_t)r * sizeof(ComponentTs))...);
            }
        }
    }
};

template <typename ArchetypeT, typename ComponentT> struct SortArchetypeNode {
    static void run(StateManager &sm)
    {
        uint32_t a = sm.archID<ArchetypeT>();
        if (sm.beforeCompact) sm.beforeCompact(a);
        Table &t = sm.tables[a];
        const WorldID *wid = (const WorldID *)t.cols[1];
        if constexpr (std::is_same_v<ComponentT, WorldID>) {
            sm.rebuild(a, true, [&](int32_t r) { return (uint64_t)(uint32_t)wid[r].idx; });
        } else {
            static_assert(sizeof(ComponentT) >= 4);
            const char *col = (const char *)sm.getArchetypeComponent<ArchetypeT, ComponentT>();
            sm.rebuild(a, true, [&](int32_t r) {
                uint32_t k;
                memcpy(&k, col + (size_t)r * sizeof(ComponentT), 4);
                return ((uint64_t)k << 32) | (uint32_t)wid[r].idx;
            });
        }
    }
};

struct ResetTmpAllocNode {
    static void run(StateManager &) {}
};

/* compacts every table that holds destroyed rows, order kept */
struct RecycleEntitiesNode {
    static void run(StateManager &sm)
    {
        for (uint32_t a = 0; a < sm.tables.size(); ++a) {
            if (!sm.tables[a].perEntity) continue;
            bool dead = false;
            for (int32_t r = 0; r < sm.tables[a].numRows && !dead; ++r) dead = !sm.rowLive(a, r);
            if (!dead) continue;
            if (sm.beforeCompact) sm.beforeCompact(a);
            sm.rebuild(a, false, nullptr);
        }
    }
};

}  // namespace madrona

#define MADRONA_BUILD_MWGPU_ENTRY(...) static_assert(true, "")
