/*
 * ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * A C ABI over the reference's own simulation translation unit (sim.cpp of the
 * project this one was modelled on, compiled as it is against the stand-in
 * engine under madrona/).  It builds the worlds the way the reference's manager
 * does (8 x 6 chunks, cellDim 1, food cap 30), runs the task graphs that
 * Sim::setupTasks built, in their order, and reads the tables back in the
 * oracle's formats (oracle/mbots_oracle.h) so that the two can be compared in
 * lock-step.  It includes nothing of oracle/mbots_oracle.c or csrc/.
 *
 * Engine-decided points the driver itself supplies:
 *   - item 7: after construction the observation rows hold species, position
 *     and health and are in (species, world) order, and each agent's sensor
 *     output index is its row there
 *   - quirk B.4 fixed: when a dead agent's row is compacted away, its
 *     observation entity goes with it (the reference leaks that row)
 *   - quirk B.13: a new agent's sensor output row starts at a row of zeros
 */
#include "sim.hpp"

#include <map>
#include <new>

namespace ma = madrona;
using namespace mbots;

namespace {

struct FoodRot {
    bool direct;        /* written by ref_set_world_state */
    uint32_t value;     /* direct: the 22-bit rotation; else the RNG counter of its draw */
};

struct RefSim {
    ma::StateManager *sm = nullptr;
    ma::ECSRegistry *reg = nullptr;
    ma::TaskGraphManager tgm;
    Sim::Config cfg{};
    SimBridge bridge{};
    std::vector<Sim *> sims;
    std::map<int32_t, FoodRot> foodRot;   /* food entity id -> its rotation's source */
    uint32_t worlds = 0;
    bool tracking = false;
};

RefSim *g_cur = nullptr;

void use(RefSim *s)
{
    g_cur = s;
    ma::mwGPU::currentStateManager() = s->sm;
}

Engine ctxOf(RefSim *s, uint32_t w) { return Engine(s->sm, s->sims[w], ma::WorldID{(int32_t)w}); }

void onAttachView(ma::Context &ctx, ma::Entity e)
{
    /* B.13: the row of zeros behind every table's last row */
    ctx.get<SensorOutputIndex>(e).idx = (uint32_t)ctx.stateManager()->maxRows;
}

void onMakeRenderable(ma::Context &ctx, ma::Entity e)
{
    RefSim *s = g_cur;
    if (!s || !s->tracking) return;
    if (ctx.loc(e).archetype != s->sm->archID<StaticObject>()) return;
    /* addFoodToChunk draws the entity's rotation next (sim.cpp:338-341);
     * ref_world_food checks that against the stored quaternion */
    Sim *sim = (Sim *)ctx.userData();
    s->foodRot[e.id] = FoodRot{false, sim->rng.counter()};
}

void beforeCompact(uint32_t arch)
{
    RefSim *s = g_cur;
    ma::StateManager &sm = *s->sm;
    if (arch != sm.archID<Agent>()) return;
    ma::Table &t = sm.tables[arch];
    auto *bridge = sm.getArchetypeComponent<Agent, AgentObservationBridge>();
    for (int32_t r = 0; r < t.numRows; ++r)
        if (!sm.rowLive(arch, r) && sm.valid(bridge[r].obsEntity)) sm.destroy(bridge[r].obsEntity);
}

ma::math::Quat foodQuat(uint32_t rot24)
{
    float u = (float)rot24 * (1.0f / 16777216.0f);
    return ma::math::Quat::angleAxis(2.f * ma::math::pi * u, ma::math::Vector3{0.f, 0.f, 1.f});
}

template <typename T> int copyOut(RefSim *s, void *out)
{
    auto *p = s->sm->getArchetypeComponent<AgentObservationArchetype, T>();
    memcpy(out, p, sizeof(T) * (size_t)s->sm->getArchetypeNumRows<AgentObservationArchetype>());
    return 0;
}
template <typename T> int copyOutRay(RefSim *s, void *out)
{
    auto *p = s->sm->getArchetypeComponent<ma::render::RaycastOutputArchetype, T>();
    memcpy(out, p, sizeof(T) * (size_t)s->sm->getArchetypeNumRows<AgentObservationArchetype>());
    return 0;
}
template <typename T> int copyIn(RefSim *s, const void *in, uint32_t rows)
{
    if (rows != s->sm->getArchetypeNumRows<AgentObservationArchetype>()) return -1;
    memcpy(s->sm->getArchetypeComponent<AgentObservationArchetype, T>(), in, sizeof(T) * (size_t)rows);
    return 0;
}
template <typename T> int copyInRay(RefSim *s, const void *in, uint32_t rows)
{
    if (rows != s->sm->getArchetypeNumRows<AgentObservationArchetype>()) return -1;
    memcpy(s->sm->getArchetypeComponent<ma::render::RaycastOutputArchetype, T>(), in, sizeof(T) * (size_t)rows);
    return 0;
}

}  // namespace

extern "C" {

/* the column numbers of oracle/mbots_oracle.h */
enum { COL_SPECIES, COL_POS, COL_HEALTH, COL_SURROUND, COL_REWARD, COL_ACTION, COL_STATS, COL_HIDDEN, COL_SEMANTIC, COL_DEPTH };

void ref_destroy(void *h)
{
    RefSim *s = (RefSim *)h;
    if (!s) return;
    for (Sim *sim : s->sims) {
        if (!sim) continue;
        sim->~Sim();
        ::operator delete((void *)sim, std::align_val_t(alignof(Sim)));
    }
    delete s->reg;
    delete s->sm;
    if (g_cur == s) {
        g_cur = nullptr;
        ma::mwGPU::currentStateManager() = nullptr;
    }
    delete s;
}

void *ref_create(uint32_t worlds, uint32_t seed, uint32_t init_agents, uint32_t max_rows)
{
    static_assert(sizeof(Action) == 24 && sizeof(HiddenState) == 64 && sizeof(StatsObservation) == 16 &&
                  sizeof(PositionObservation) == 8 && sizeof(SurroundingObservation) == 8 && sizeof(SpeciesCount) == 16);
    if (worlds == 0) return nullptr;
    RefSim *s = new RefSim;
    s->worlds = worlds;
    /* every table is allocated once at this many rows (+ one of padding) */
    uint32_t need = worlds * 64u + 64u;
    if (max_rows < need) max_rows = need;
    s->sm = new ma::StateManager(worlds, (int32_t)max_rows);
    s->reg = new ma::ECSRegistry(s->sm);
    use(s);
    ma::render::RenderingSystem::onAttachView() = onAttachView;
    ma::render::RenderingSystem::onMakeRenderable() = onMakeRenderable;
    s->sm->beforeCompact = beforeCompact;

    /* mgr.cpp's constants */
    s->cfg.initRandKey = ma::rand::initKey(seed);
    s->cfg.numChunksX = 8;
    s->cfg.numChunksY = 6;
    s->cfg.cellDim = 1.f;
    s->cfg.renderBridge = nullptr;
    s->cfg.simBridge = &s->bridge;
    s->cfg.totalAllowedFood = 30;
    s->cfg.initNumAgentsPerWorld = init_agents;

    Sim::registerTypes(*s->reg, s->cfg);
    Sim::setupTasks(s->tgm, s->cfg);

    s->sims.assign(worlds, nullptr);
    for (uint32_t w = 0; w < worlds; ++w) {
        for (uint32_t a : s->reg->singletons) s->sm->addRows(a, (int32_t)w, 1);
        void *mem = ::operator new(sizeof(Sim), std::align_val_t(alignof(Sim)));
        memset(mem, 0, sizeof(Sim));
        s->sims[w] = (Sim *)mem;
        s->sm->worldData[w] = mem;
        Engine ctx = ctxOf(s, w);
        new (mem) Sim(ctx, s->cfg, Sim::WorldInit{});
    }
    s->tgm.run(TaskGraphID::Init, *s->sm);

    /* the first export */
    ma::StateManager &sm = *s->sm;
    sm.rebuild(sm.archID<Agent>(), false, nullptr);
    uint32_t n = sm.getArchetypeNumRows<Agent>();
    auto *wid = (ma::WorldID *)sm.tables[sm.archID<Agent>()].cols[1];
    for (uint32_t r = 0; r < n; ++r) {
        Engine ctx = ctxOf(s, (uint32_t)wid[r].idx);
        ma::Entity obs = sm.getArchetypeComponent<Agent, AgentObservationBridge>()[r].obsEntity;
        const auto &pos = sm.getArchetypeComponent<Agent, ma::base::Position>()[r];
        ctx.get<SpeciesObservation>(obs).speciesID = sm.getArchetypeComponent<Agent, Species>()[r].speciesID;
        ctx.get<PositionObservation>(obs).pos = ma::math::Vector2{pos.x, pos.y};
        ctx.get<HealthObservation>(obs).v = sm.getArchetypeComponent<Agent, Health>()[r].v;
    }
    ma::SortArchetypeNode<AgentObservationArchetype, SpeciesObservation>::run(sm);
    /* the first agents' sensor output rows are their export rows (all zero yet) */
    for (uint32_t r = 0; r < n; ++r)
        sm.getArchetypeComponent<Agent, SensorOutputIndex>()[r].idx =
            (uint32_t)sm.loc(sm.getArchetypeComponent<Agent, AgentObservationBridge>()[r].obsEntity).row;
    s->bridge.totalNumAgents = n;
    s->bridge.agentWorldOffsets = sm.getArchetypeWorldOffsets<Agent>();
    s->bridge.agentWorldCounts = sm.getArchetypeWorldCounts<Agent>();
    s->tracking = true;
    return s;
}

void ref_step(void *h)
{
    RefSim *s = (RefSim *)h;
    use(s);
    s->tgm.run(TaskGraphID::Step, *s->sm);
}

void ref_sensor(void *h)
{
    RefSim *s = (RefSim *)h;
    use(s);
    s->tgm.run(TaskGraphID::Sensor, *s->sm);
}

void ref_shift_observations(void *h)
{
    RefSim *s = (RefSim *)h;
    use(s);
    s->tgm.run(TaskGraphID::ShiftObservations, *s->sm);
}

uint32_t ref_num_agents(void *h) { return ((RefSim *)h)->sm->getArchetypeNumRows<AgentObservationArchetype>(); }

/* what bridgeSyncSystem last published */
uint32_t ref_bridge_total(void *h) { return ((RefSim *)h)->bridge.totalNumAgents; }

int ref_read_column(void *h, int col, int is_prev, void *out)
{
    RefSim *s = (RefSim *)h;
    use(s);
    switch (col) {
    case COL_SPECIES: return is_prev ? copyOut<PrevSpeciesObservation>(s, out) : copyOut<SpeciesObservation>(s, out);
    case COL_POS: return is_prev ? copyOut<PrevPositionObservation>(s, out) : copyOut<PositionObservation>(s, out);
    case COL_HEALTH: return is_prev ? copyOut<PrevHealthObservation>(s, out) : copyOut<HealthObservation>(s, out);
    case COL_SURROUND: return is_prev ? copyOut<PrevSurroundingObservation>(s, out) : copyOut<SurroundingObservation>(s, out);
    case COL_REWARD: return is_prev ? copyOut<PrevReward>(s, out) : copyOut<Reward>(s, out);
    case COL_ACTION: return is_prev ? copyOut<PrevAction>(s, out) : copyOut<Action>(s, out);
    case COL_STATS: return is_prev ? copyOut<PrevStatsObservation>(s, out) : copyOut<StatsObservation>(s, out);
    case COL_HIDDEN: return is_prev ? copyOut<PrevHiddenState>(s, out) : copyOut<HiddenState>(s, out);
    case COL_SEMANTIC:
        return is_prev ? copyOutRay<ma::render::PrevSemanticOutputBuffer>(s, out)
                       : copyOutRay<ma::render::SemanticOutputBuffer>(s, out);
    case COL_DEPTH:
        return is_prev ? copyOutRay<ma::render::PrevDepthOutputBuffer>(s, out)
                       : copyOutRay<ma::render::DepthOutputBuffer>(s, out);
    default: return -1;
    }
}

/* current Action / HiddenState (a policy's writes) and the current sensor rows
 * (the renderer's), `rows` export rows each */
int ref_write_column(void *h, int col, const void *in, uint32_t rows)
{
    RefSim *s = (RefSim *)h;
    use(s);
    switch (col) {
    case COL_ACTION: return copyIn<Action>(s, in, rows);
    case COL_HIDDEN: return copyIn<HiddenState>(s, in, rows);
    case COL_SEMANTIC: return copyInRay<ma::render::SemanticOutputBuffer>(s, in, rows);
    case COL_DEPTH: return copyInRay<ma::render::DepthOutputBuffer>(s, in, rows);
    default: return -1;
    }
}

/* the SpeciesCount column as speciesInfoSync wrote it: [W][4], before respawns */
void ref_species_count(void *h, int32_t *out)
{
    RefSim *s = (RefSim *)h;
    use(s);
    memcpy(out, s->sm->getArchetypeComponent<SpeciesInfoArchetype, SpeciesCount>(), sizeof(SpeciesCount) * s->worlds);
}

/* through the SimBridge pointers */
void ref_world_counts(void *h, int32_t *counts, int32_t *offsets)
{
    RefSim *s = (RefSim *)h;
    for (uint32_t w = 0; w < s->worlds; ++w) {
        if (counts) counts[w] = s->bridge.agentWorldCounts[w];
        if (offsets) offsets[w] = s->bridge.agentWorldOffsets[w];
    }
}

/* the Agent archetype's SensorOutputIndex column, world-major */
void ref_sensor_index(void *h, int32_t *out)
{
    RefSim *s = (RefSim *)h;
    use(s);
    memcpy(out, s->sm->getArchetypeComponent<Agent, SensorOutputIndex>(), 4 * (size_t)s->sm->getArchetypeNumRows<Agent>());
}

int32_t ref_world_state(void *h, uint32_t w, float *xy, float *rot, int32_t *species, int32_t *health)
{
    RefSim *s = (RefSim *)h;
    use(s);
    ma::StateManager &sm = *s->sm;
    if (w >= s->worlds) return -1;
    int32_t off = sm.getArchetypeWorldOffsets<Agent>()[w], n = sm.getArchetypeWorldCounts<Agent>()[w];
    for (int32_t i = 0; i < n; ++i) {
        const auto &p = sm.getArchetypeComponent<Agent, ma::base::Position>()[off + i];
        const auto &q = sm.getArchetypeComponent<Agent, ma::base::Rotation>()[off + i];
        if (xy) { xy[2 * i] = p.x; xy[2 * i + 1] = p.y; }
        if (rot) { rot[2 * i] = q.w; rot[2 * i + 1] = q.z; }
        if (species) species[i] = (int32_t)sm.getArchetypeComponent<Agent, Species>()[off + i].speciesID;
        if (health) health[i] = sm.getArchetypeComponent<Agent, Health>()[off + i].v;
    }
    return n;
}

int32_t ref_current_food(void *h, uint32_t w) { return ((RefSim *)h)->sims[w]->currentNumFood.load_relaxed(); }

/* orc_world_food's format: (chunk, x, y, 22-bit rotation) per live package in
 * (chunk, package) order.  -1: a package's entity does not hold the rotation
 * its draw gives (or has no recorded draw). */
int32_t ref_world_food(void *h, uint32_t w, int32_t *out)
{
    RefSim *s = (RefSim *)h;
    use(s);
    Engine ctx = ctxOf(s, w);
    Sim &sim = *s->sims[w];
    int32_t k = 0;
    for (uint32_t c = 0; c < sim.numChunksX * sim.numChunksY; ++c) {
        ChunkInfo *ci = sim.getChunkInfo(ctx, (int32_t)c);
        for (uint32_t p = 0; p < ChunkInfo::kMaxFoodPackages; ++p) {
            FoodPackage &pk = ci->foodPackages[p];
            if (pk.numFood.load_relaxed() == 0) continue;
            auto it = s->foodRot.find(pk.foodEntity.id);
            if (it == s->foodRot.end() || !s->sm->valid(pk.foodEntity)) return -1;
            uint32_t rot24 = it->second.direct ? it->second.value : (ma::rand::bits32(sim.rng.key(), it->second.value) >> 8);
            ma::math::Quat want = foodQuat(rot24), got = ctx.get<ma::base::Rotation>(pk.foodEntity);
            if (memcmp(&want, &got, sizeof(want)) != 0) return -1;
            const auto &pos = ctx.get<ma::base::Position>(pk.foodEntity);
            int32_t x = (int32_t)(c % sim.numChunksX) * (int32_t)ChunkInfo::kChunkWidth + pk.x;
            int32_t y = (int32_t)(c / sim.numChunksX) * (int32_t)ChunkInfo::kChunkWidth + pk.y;
            if (pos.x != (float)x || pos.y != (float)y) return -1;   /* the entity stands on its cell */
            out[4 * k + 0] = (int32_t)c;
            out[4 * k + 1] = x;
            out[4 * k + 2] = y;
            out[4 * k + 3] = (int32_t)(rot24 & 0x3FFFFFu);
            ++k;
        }
    }
    return k;
}

/* each agent's finder hit for the next step: slots[i] is the hit agent's slot
 * in world w, or -1 */
int ref_set_finder(void *h, uint32_t w, const int32_t *slots, uint32_t n)
{
    RefSim *s = (RefSim *)h;
    use(s);
    ma::StateManager &sm = *s->sm;
    if (w >= s->worlds) return -1;
    int32_t off = sm.getArchetypeWorldOffsets<Agent>()[w], cnt = sm.getArchetypeWorldCounts<Agent>()[w];
    if ((int32_t)n != cnt) return -1;
    Engine ctx = ctxOf(s, w);
    auto *ents = (ma::Entity *)sm.tables[sm.archID<Agent>()].cols[0];
    for (int32_t i = 0; i < cnt; ++i) {
        if (slots[i] >= cnt) return -1;
        ma::Entity cam = sm.getArchetypeComponent<Agent, ma::render::RenderCamera>()[off + i].cameraEntity;
        ctx.get<ma::render::FinderOutputBuffer>(cam).out.hitEntity = slots[i] < 0 ? ma::Entity::none() : ents[off + slots[i]];
    }
    return 0;
}

/* orc_set_world_state's arguments: positions and (w, z) rotations of the live
 * agents, and the world's food replaced by the packages given */
int ref_set_world_state(void *h, uint32_t w, const float *xy_rwrz, uint32_t n_agents, const int32_t *food, uint32_t n_food)
{
    RefSim *s = (RefSim *)h;
    use(s);
    ma::StateManager &sm = *s->sm;
    if (w >= s->worlds) return -1;
    int32_t off = sm.getArchetypeWorldOffsets<Agent>()[w], cnt = sm.getArchetypeWorldCounts<Agent>()[w];
    if ((int32_t)n_agents != cnt || n_food > s->cfg.totalAllowedFood) return -1;
    Sim &sim = *s->sims[w];
    const int32_t cw = (int32_t)ChunkInfo::kChunkWidth, ncx = (int32_t)sim.numChunksX, nch = ncx * (int32_t)sim.numChunksY;
    std::vector<uint32_t> used((size_t)nch, 0u);
    for (uint32_t k = 0; k < n_food; ++k) {
        int32_t c = food[4 * k], lx = food[4 * k + 1] - (c % ncx) * cw, ly = food[4 * k + 2] - (c / ncx) * cw;
        if (c < 0 || c >= nch || lx < 0 || lx >= cw || ly < 0 || ly >= cw) return -1;
        if (food[4 * k + 3] < 0 || food[4 * k + 3] >= (1 << 22)) return -1;
        if (++used[(size_t)c] > ChunkInfo::kMaxFoodPackages) return -1;
    }
    for (int32_t i = 0; i < cnt; ++i) {
        auto &p = sm.getArchetypeComponent<Agent, ma::base::Position>()[off + i];
        p.x = xy_rwrz[4 * i];
        p.y = xy_rwrz[4 * i + 1];
        sm.getArchetypeComponent<Agent, ma::base::Rotation>()[off + i] =
            ma::math::Quat{xy_rwrz[4 * i + 2], 0.f, 0.f, xy_rwrz[4 * i + 3]};
    }
    Engine ctx = ctxOf(s, w);
    s->tracking = false;
    for (int32_t c = 0; c < nch; ++c) {
        ChunkInfo *ci = sim.getChunkInfo(ctx, c);
        for (uint32_t p = 0; p < ChunkInfo::kMaxFoodPackages; ++p) {
            FoodPackage &pk = ci->foodPackages[p];
            if (pk.numFood.load_relaxed() != 0) {
                s->foodRot.erase(pk.foodEntity.id);
                ctx.destroyRenderableEntity(pk.foodEntity);
            }
            pk.numFood.store_relaxed(0);
            pk.x = 0;
            pk.y = 0;
        }
    }
    std::fill(used.begin(), used.end(), 0u);
    for (uint32_t k = 0; k < n_food; ++k) {
        int32_t c = food[4 * k];
        FoodPackage &pk = sim.getChunkInfo(ctx, c)->foodPackages[used[(size_t)c]++];
        pk.x = (uint8_t)(food[4 * k + 1] - (c % ncx) * cw);
        pk.y = (uint8_t)(food[4 * k + 2] - (c / ncx) * cw);
        pk.numFood.store_relaxed(1);
        ma::Entity e = ctx.makeRenderableEntity<StaticObject>();
        ctx.get<ma::base::Position>(e) = ma::math::Vector3{(float)food[4 * k + 1], (float)food[4 * k + 2], 1.f};
        ctx.get<ma::base::Rotation>(e) = foodQuat((uint32_t)food[4 * k + 3]);
        ctx.get<ma::base::Scale>(e) = ma::math::Diag3x3{1.f, 1.f, 1.f};
        ctx.get<ma::base::ObjectID>(e).idx = (int32_t)SimObject::Food;
        pk.foodEntity = e;
        s->foodRot[e.id] = FoodRot{true, (uint32_t)food[4 * k + 3]};
    }
    sim.currentNumFood.store_relaxed((int32_t)n_food);
    s->tracking = true;
    return 0;
}

}  // extern "C"
