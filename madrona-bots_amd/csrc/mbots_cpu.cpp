// mbots_cpu.cpp -- the CPU execution mode behind the same C ABI (mbots.h,
// MBOTS_EXEC_CPU): BASELINE config 1 ("64 worlds, ExecMode::CPU via
// learn/env.py, runs without a GPU"; learn/env.py:12-15 selects it when no
// GPU is present).  Systems follow the HIP kernels of mbots_kernels.hip
// system for system (sim.cpp:1061-1220), one world per task on host threads;
// every float expression is the shared host+device one (mbots_device.hpp,
// mbots_ray.hpp), so the results are bit-identical to the HIP path.
#include "mbots_cpu.hpp"
#include "mbots_ray.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <type_traits>

namespace mbots {
namespace cpu {

namespace {

constexpr uint32_t kLive = 1u << 8;   // per-package image: x | y << 4 | live << 8
constexpr uint8_t F_HIT_FRIENDLY = 1, F_HIT_ENEMY = 2, F_ATE = 4, F_REPRO = 8, F_ALIVE = 16,
                  F_BREED = 32;

// one world's working image (the K1 LDS image of mbots_kernels.hip)
struct Slot {
    float x, y, rw, rz, s0, s1;
    int32_t accum, row, sp, fd;
    uint8_t fl;
};

inline uint32_t rng_draw(uint2 key, uint32_t ctr) { return threefry2x32(key.x, key.y, ctr, 0u).x; }

// pinhole offsets u = (2k + 1) / 24 - 1 (forward), (2k' + 1) / 8 - 1 (backward)
// as one rounding, the kernels' u_of
inline float ray_u(int k)
{
    return k < 24 ? (float)(2 * k - 23) * (1.0f / 24.0f) : (float)(2 * (k - 24) - 7) * 0.125f;
}

template <typename T> void put(std::vector<T> &v, size_t n) { v.assign(n, T{}); }

}  // namespace

void Table::resize(size_t rows)
{
    put(species, rows); put(health, rows); put(action, rows * 6); put(stats, rows * 4);
    put(pspecies, rows); put(phealth, rows); put(paction, rows * 6); put(pstats, rows * 4);
    put(pos, rows * 2); put(sur, rows * 2); put(reward, rows); put(hidden, rows * kHidden);
    put(ppos, rows * 2); put(psur, rows * 2); put(preward, rows); put(phidden, rows * kHidden);
    put(sem, rows * kSensor); put(psem, rows * kSensor);
    put(depth, rows * kSensor); put(pdepth, rows * kSensor);
}

template <typename F> void Sim::for_worlds(F &&fn) const
{
    const unsigned T = std::max(1u, std::min<unsigned>(threads_, W_));
    if (T == 1) {
        for (uint32_t w = 0; w < W_; ++w) fn(w);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(T);
    for (unsigned t = 0; t < T; ++t) {
        const uint32_t lo = (uint32_t)((uint64_t)W_ * t / T), hi = (uint32_t)((uint64_t)W_ * (t + 1) / T);
        th.emplace_back([&fn, lo, hi] {
            for (uint32_t w = lo; w < hi; ++w) fn(w);
        });
    }
    for (auto &t : th) t.join();
}

Sim::Sim(const mbots_config &cfg)
    : cfg_(cfg), W_(cfg.num_worlds + ((cfg.flags & MBOTS_FLAG_SHARD_GHOST) ? 1u : 0u)), Wx_(cfg.num_worlds),
      cap_(cfg.agent_capacity), A_(cfg.init_num_agents_per_world)
{
    const char *e = getenv("MBOTS_CPU_THREADS");
    // default: the machine's threads up to 16 (a GPU box's per-GPU CPU share;
    // MBOTS_CPU_THREADS overrides, e.g. bench.py's all-core baseline).  Each
    // phase starts its threads on contiguous world ranges: a persistent pool
    // with dynamic chunks measured 2x slower on the GPU box (16-CPU cgroup)
    threads_ = e ? (unsigned)atoi(e) : std::min(16u, std::thread::hardware_concurrency());
    if (threads_ == 0) threads_ = 1;
    const size_t rows = (size_t)W_ * cap_;
    for (auto *v : {&x_, &y_, &rw_, &rz_, &sur0_, &sur1_}) put(*v, rows);
    for (auto *v : {&species_, &health_, &finder_, &obsrow_}) put(*v, rows);
    put(stats_, rows);
    for (auto *v : {&n_, &cur_food_, &world_off_}) put(*v, W_);
    put(scount_, (size_t)W_ * kNumSpecies);
    put(row_base_, (size_t)W_ * kNumSpecies);
    put(key_, W_);
    put(ctr_, W_);
    put(overflow_, W_);
    put(food_rot_, (size_t)W_ * kNumPkg);
    put(food_, (size_t)W_ * kNumChunks);
    put(sreward_, (size_t)W_ * kNumSpecies);
    T_[0].resize(rows);
    T_[1].resize(rows);
    put(zeros_rows_, rows);
    put(reset_flags_, W_);
    put(episode_, W_);
    put(age_, W_);
    put(reset_mark_, W_);
    put(sensor_index_, rows);
    put(src_of_, rows);
    // Sim::Sim + initWorld (sim.cpp:1232-1256, :233-275), then the first export
    for_worlds([&](uint32_t w) { init_world(w); });
    scan();
    agent_steps_ = 0;   // the initial population is not a step
    for_worlds([&](uint32_t w) { export_world(w, T_[1], T_[0], true); });
    tb_ = 0;
}

// episode e of global world gw is keyed threefry2x32(seed, 0, e, gw):
// split_i(initKey, episode, world), sim.cpp:1236-1240.  reset: a world's
// re-initialisation between steps (reset_pass) also clears what a fresh Sim
// holds as zeros
void Sim::init_world(uint32_t w, uint32_t episode, bool reset)
{
    const size_t base = (size_t)w * cap_;
    const uint2 key = threefry2x32(cfg_.rand_seed, 0u, episode, cfg_.world_offset + w);
    if (reset) {
        for (uint32_t i = 0; i < A_; ++i) {
            sur0_[base + i] = sur1_[base + i] = 0.0f;
            stats_[base + i] = 0u;
        }
        std::fill_n(food_.begin() + (size_t)w * kNumChunks, kNumChunks, 0ull);
        std::fill_n(food_rot_.begin() + (size_t)w * kNumPkg, kNumPkg, 0u);
        std::fill_n(sreward_.begin() + (size_t)w * kNumSpecies, kNumSpecies, 0.0f);
        cur_food_[w] = 0;
    }
    for (uint32_t i = 0; i < A_; ++i) {
        x_[base + i] = u01(rng_draw(key, 2u * i)) * kLx;
        y_[base + i] = u01(rng_draw(key, 2u * i + 1u)) * kLy;
        rw_[base + i] = 1.0f;
        rz_[base + i] = 0.0f;
        species_[base + i] = (int32_t)(i % kNumSpecies) + 1;
        health_[base + i] = 100;
        finder_[base + i] = -1;
        obsrow_[base + i] = -1;
    }
    for (int s = 0; s < kNumSpecies; ++s)
        scount_[(size_t)w * kNumSpecies + s] = (int32_t)(A_ / kNumSpecies + ((uint32_t)s < A_ % kNumSpecies ? 1 : 0));
    key_[w] = key;
    ctr_[w] = 2u * A_;
    n_[w] = (int32_t)A_;
}

// resetChunkInfoSystem, addFoodSystem, actionSystem, healthSync,
// updateSurroundingObservation, speciesTrackerUpdate, speciesInfoSync +
// respawn, SortArchetypeNode<Agent, WorldID> (sim.cpp:1061-1132) -- K1
void Sim::world_step(uint32_t w, const Table &cur)
{
    const size_t base = (size_t)w * cap_;
    const int n0 = n_[w];
    thread_local std::vector<Slot> L;
    L.resize(cap_);
    for (int i = 0; i < n0; ++i) {
        const size_t s = base + i;
        L[i] = Slot{x_[s], y_[s], rw_[s], rz_[s], 0.0f, 0.0f, health_[s], obsrow_[s], species_[s],
                    finder_[s], F_ALIVE};
    }
    uint16_t pk[kNumPkg];
    uint32_t chunk[kNumChunks] = {};   // ChunkInfo: numAgents << 16 | totalSpeed
    for (int c = 0; c < kNumChunks; ++c) {
        const uint64_t rec = food_[(size_t)w * kNumChunks + c];
        for (int q = 0; q < kMaxPkg; ++q)
            pk[c * kMaxPkg + q] = (uint16_t)(((rec >> (8 * q)) & 0xFFu) | (((rec >> (40 + q)) & 1u) << 8));
    }
    const uint2 key = key_[w];
    uint32_t ctr = ctr_[w];
    int32_t cur_food = cur_food_[w];
    auto draw = [&] { return rng_draw(key, ctr++); };

    // ---- addFoodSystem (sim.cpp:363-387) + addFoodToChunk (:308-361) ----
    if (sample_i32(draw(), 0, 10) == 0) {
        uint32_t nfood = (uint32_t)sample_i32(draw(), 1, 3);
        const uint32_t diff = (uint32_t)kFoodCap - (uint32_t)cur_food;
        if (diff < nfood) nfood = diff;
        for (uint32_t f = 0; f < nfood; ++f) {
            const uint32_t cx = (uint32_t)sample_i32(draw(), 0, kChunksX);
            const uint32_t cy = (uint32_t)sample_i32(draw(), 0, kChunksY);
            const int c = (int)(cx + cy * kChunksX);
            draw();   // two unused draws (sim.cpp:311-312)
            draw();
            for (int q = 0; q < kMaxPkg; ++q) {
                if ((pk[c * kMaxPkg + q] & kLive) == 0u) {
                    const uint32_t rx = (uint32_t)sample_i32(draw(), 0, kChunkW);
                    const uint32_t ry = (uint32_t)sample_i32(draw(), 0, kChunkW);
                    // food entity rotation (sim.cpp:338-341): 22-bit quarter turn
                    food_rot_[((size_t)w * kMaxPkg + q) * kNumChunks + c] = (draw() >> 8) & 0x3FFFFFu;
                    pk[c * kMaxPkg + q] = (uint16_t)((rx & 15u) | ((ry & 15u) << 4) | kLive);
                    cur_food += 1;
                    break;
                }
            }
        }
    }

    // ---- actionSystem (sim.cpp:419-502) ----
    for (int i = 0; i < n0; ++i) {
        Slot &a = L[i];
        int32_t act[6] = {0, 0, 0, 0, 0, 0};
        if (a.row >= 0) memcpy(act, &cur.action[(size_t)a.row * 6], sizeof(act));
        uint8_t fl = F_ALIVE | (act[5] ? F_BREED : 0);
        if (act[4] && a.fd >= 0) {
            L[a.fd].accum += -50;
            fl |= (L[a.fd].sp == a.sp) ? F_HIT_FRIENDLY : F_HIT_ENEMY;
        }
        float rw = a.rw, rz = a.rz;
        if (act[2]) {
            const float nw = rw * kRotC - rz * kRotS, nz = rw * kRotS + rz * kRotC;
            rw = nw; rz = nz;
        } else if (act[3]) {
            const float nw = rw * kRotC - rz * (-kRotS), nz = rw * (-kRotS) + rz * kRotC;
            rw = nw; rz = nz;
        }
        float x = a.x, y = a.y;
        const float ox = x, oy = y;
        float dx, dy;
        heading(rw, rz, dx, dy);
        if (act[0]) { x = x + dx; y = y + dy; }
        else if (act[1]) { x = x - dx; y = y - dy; }
        x = fmin_std(kLx - 1.0f, fmax_std(0.0f, x));
        y = fmin_std(kLy - 1.0f, fmax_std(0.0f, y));
        const float ddx = x - ox, ddy = y - oy;
        const float len = sqrtf(ddx * ddx + ddy * ddy);
        const int32_t ci = chunk_index(floorf((x / 1.0f) / 16.0f), floorf((y / 1.0f) / 16.0f));
        chunk[ci] += (1u << 16) + (uint32_t)(len * 2.0f);
        a.x = x; a.y = y; a.rw = rw; a.rz = rz;
        a.fl = fl;
    }

    // ---- healthSync (sim.cpp:505-581): the agents on a cell consume its live
    // packages in slot order (FoodPackage::consume, sim.inl:76-99) ----
    int n1 = n0, consumed = 0;
    uint32_t ovf = 0;
    for (int i = 0; i < n0; ++i) {
        Slot &a = L[i];
        const float chx = (a.x / 1.0f) / 16.0f, chy = (a.y / 1.0f) / 16.0f;
        const uint32_t cx = (uint8_t)(16.0f * (chx - floorf(chx)));
        const uint32_t cy = (uint8_t)(16.0f * (chy - floorf(chy)));
        const int32_t ci = chunk_index(chx, chy);
        const uint32_t cell = cx | (cy << 4) | kLive;
        int32_t h = a.accum;
        uint8_t fl = a.fl;
        for (int q = 0; q < kMaxPkg; ++q) {
            if (pk[ci * kMaxPkg + q] == cell) {
                pk[ci * kMaxPkg + q] &= (uint16_t)0xFFu;   // numFood 1 -> 0
                consumed += 1;
                h = (int32_t)((float)h + 20.0f);
                fl |= F_ATE;
                break;
            }
        }
        if ((fl & F_BREED) && h > 10 && a.fd >= 0 && L[a.fd].sp == a.sp) {   // :547-569
            h -= 40;
            fl |= F_REPRO;
            if (n1 < (int)cap_) {
                L[n1] = Slot{a.x, a.y, 1.0f, 0.0f, 0.0f, 0.0f, 50, -1, a.sp, -1, F_ALIVE};
                n1 += 1;
            } else {
                ovf += 1;
            }
        }
        if (h <= 0) fl &= (uint8_t)~F_ALIVE;
        a.accum = h;
        a.fl = fl;
    }
    cur_food -= consumed;

    // ---- updateSurroundingObservation (sim.cpp:583-654) + tracker (:719-734) ----
    uint32_t cnt[kNumSpecies] = {}, hsum[kNumSpecies] = {};
    for (int i = 0; i < n1; ++i) {
        Slot &a = L[i];
        if (!(a.fl & F_ALIVE)) continue;
        float cpx = a.x / 1.0f, cpy = a.y / 1.0f;
        cpx = cpx - 16.0f * 0.5f;
        cpy = cpy - 16.0f * 0.5f;
        const float chx = cpx / 16.0f, chy = cpy / 16.0f;
        const float x0 = floorf(chx), y0 = floorf(chy), x1 = ceilf(chx), y1 = ceilf(chy);
        const int32_t i00 = chunk_index(x0, y0), i10 = chunk_index(x1, y0);
        const int32_t i01 = chunk_index(x0, y1), i11 = chunk_index(x1, y1);
        const float xi = chx - x0, yi = chy - y0;
        const uint32_t c00 = i00 >= 0 ? chunk[i00] : 0u, c10 = i10 >= 0 ? chunk[i10] : 0u;
        const uint32_t c01 = i01 >= 0 ? chunk[i01] : 0u, c11 = i11 >= 0 ? chunk[i11] : 0u;
        const float n00 = (float)(c00 >> 16), n10 = (float)(c10 >> 16);
        const float n01 = (float)(c01 >> 16), n11 = (float)(c11 >> 16);
        const float s00 = (float)(c00 & 0xFFFFu), s10 = (float)(c10 & 0xFFFFu);
        const float s01 = (float)(c01 & 0xFFFFu), s11 = (float)(c11 & 0xFFFFu);
        const float nx0 = xi * n10 + (1.0f - xi) * n00;
        const float nx1 = xi * n11 + (1.0f - xi) * n01;
        const float sx0 = xi * s10 + (1.0f - xi) * s00;
        const float sx1 = xi * s11 + (1.0f - xi) * s01;
        a.s0 = yi * nx1 + (1.0f - yi) * nx0;
        a.s1 = yi * sx1 + (1.0f - yi) * sx0;
        cnt[a.sp - 1] += 1u;
        hsum[a.sp - 1] += (uint32_t)a.accum;
    }

    // ---- speciesInfoSync (sim.cpp:791-838) + respawn ----
    const uint32_t per_species = A_ / kNumSpecies;
    int n2 = n1;
    for (int s = 0; s < kNumSpecies; ++s) {
        const uint32_t count = cnt[s];
        float avg = (float)hsum[s] / (float)count;
        if (count == 0) avg = 0.0f;
        sreward_[(size_t)w * kNumSpecies + s] = (float)count / (float)A_ + avg / 100.0f - 2.0f;
        for (uint32_t e = count; e < per_species; ++e) {
            const float x = u01(draw()) * kLx;
            const float y = u01(draw()) * kLy;
            if (n2 < (int)cap_) {
                L[n2] = Slot{x, y, 1.0f, 0.0f, 0.0f, 0.0f, 100, -1, s + 1, -1, F_ALIVE};
                n2 += 1;
            } else {
                ovf += 1;
            }
        }
    }

    // ---- compaction (SortArchetypeNode<Agent, WorldID>, sim.cpp:1129) ----
    int nn = 0;
    int32_t sc[kNumSpecies] = {};
    for (int i = 0; i < n2; ++i) {
        const Slot &a = L[i];
        if (!(a.fl & F_ALIVE)) continue;
        const size_t d = base + nn++;
        x_[d] = a.x; y_[d] = a.y; rw_[d] = a.rw; rz_[d] = a.rz;
        species_[d] = a.sp;
        health_[d] = a.accum;
        obsrow_[d] = i < n0 ? a.row : -1;   // newborns / respawns: no row yet
        sur0_[d] = a.s0; sur1_[d] = a.s1;
        stats_[d] = a.fl & 0xFu;
        sc[a.sp - 1] += 1;
    }
    for (int c = 0; c < kNumChunks; ++c) {
        uint64_t rec = 0;
        for (int q = 0; q < kMaxPkg; ++q) {
            const uint32_t p = pk[c * kMaxPkg + q];
            rec |= (uint64_t)(p & 0xFFu) << (8 * q);
            rec |= (uint64_t)((p >> 8) & 1u) << (40 + q);
        }
        food_[(size_t)w * kNumChunks + c] = rec;
    }
    for (int s = 0; s < kNumSpecies; ++s) scount_[(size_t)w * kNumSpecies + s] = sc[s];
    n_[w] = nn;
    ctr_[w] = ctr;
    cur_food_[w] = cur_food;
    overflow_[w] += ovf;
}

// species-major row offsets (SortArchetypeNode<Obs, Species>, sim.cpp:1147-1149,
// rows ordered (species, world, slot)); world-major agent offsets -- K2
void Sim::scan()
{
    int32_t tot[kNumSpecies] = {};
    for (uint32_t w = 0; w < Wx_; ++w)
        for (int s = 0; s < kNumSpecies; ++s) tot[s] += scount_[(size_t)w * kNumSpecies + s];
    int32_t run[kNumSpecies];
    int32_t acc = 0;
    for (int s = 0; s < kNumSpecies; ++s) { run[s] = acc; acc += tot[s]; }
    int32_t off = 0;
    for (uint32_t w = 0; w < Wx_; ++w) {
        for (int s = 0; s < kNumSpecies; ++s) {
            row_base_[(size_t)w * kNumSpecies + s] = run[s];
            run[s] += scount_[(size_t)w * kNumSpecies + s];
        }
        world_off_[w] = off;
        off += n_[w];
    }
    for (uint32_t w = Wx_; w < W_; ++w) {   // the shard ghost: rows after every exported row
        int32_t r = acc;
        for (int s = 0; s < kNumSpecies; ++s) {
            row_base_[(size_t)w * kNumSpecies + s] = r;
            r += scount_[(size_t)w * kNumSpecies + s];
        }
        world_off_[w] = acc;
    }
    N_ = (uint32_t)acc;
    totals_[0] = N_;
    for (int s = 0; s < kNumSpecies; ++s) totals_[1 + s] = (uint32_t)tot[s];
    agent_steps_ += N_;
}

// updateObservations (sim.cpp:687-717), rewardSystem setting 8 (:942-956), and
// the columns that travel with an observation row through the species sort
// (Action, HiddenState, Prev*, the prev sensor, updateSensorOutputIdx
// :736-789) -- K3a + K4, eager
void Sim::export_world(uint32_t w, const Table &cur, Table &nxt, bool init)
{
    const size_t base = (size_t)w * cap_;
    const int n = n_[w];
    const float *rew = &sreward_[(size_t)w * kNumSpecies];
    const bool fixed = (cfg_.flags & MBOTS_FLAG_REWARD_FIXED) != 0;
    const bool fixd = (cfg_.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    // faithful B.3: rewards[4] reads the next SpeciesInfo row's rewards[0]
    const float next_r0 = (w + 1 < W_) ? sreward_[(size_t)(w + 1) * kNumSpecies] : 0.0f;
    int32_t rank[kNumSpecies] = {};
    auto mv = [](auto &dst, const auto &src, size_t r, int32_t o, size_t k) {
        for (size_t c = 0; c < k; ++c) dst[r * k + c] = o >= 0 ? src[(size_t)o * k + c] : 0;
    };
    for (int i = 0; i < n; ++i) {
        const size_t s = base + i;
        const int32_t sp = species_[s];
        const size_t r = (size_t)(row_base_[(size_t)w * kNumSpecies + sp - 1] + rank[sp - 1]++);
        const int32_t o = obsrow_[s];
        const int32_t h = health_[s];
        const uint32_t st = init ? 0u : stats_[s];
        nxt.species[r] = sp;
        nxt.pos[r * 2] = x_[s];
        nxt.pos[r * 2 + 1] = y_[s];
        nxt.health[r] = h;
        nxt.sur[r * 2] = init ? 0.0f : sur0_[s];
        nxt.sur[r * 2 + 1] = init ? 0.0f : sur1_[s];
        for (int b = 0; b < 4; ++b) nxt.stats[r * 4 + b] = (int32_t)((st >> b) & 1u);
        float rv = 0.0f;
        if (!init) {
            const float sr = fixed ? rew[sp - 1] : (sp < kNumSpecies ? rew[sp] : next_r0);
            rv = sr + (float)h / 100.0f - 0.5f;
            if (st & F_ATE) rv += 10.0f;
            if (st & F_REPRO) rv += 10.0f;
            if (st & F_HIT_ENEMY) rv += 15.0f;
        }
        nxt.reward[r] = rv;
        mv(nxt.action, cur.action, r, o, 6);
        mv(nxt.hidden, cur.hidden, r, o, kHidden);
        mv(nxt.pspecies, cur.pspecies, r, o, 1);
        mv(nxt.ppos, cur.ppos, r, o, 2);
        mv(nxt.phealth, cur.phealth, r, o, 1);
        mv(nxt.psur, cur.psur, r, o, 2);
        mv(nxt.preward, cur.preward, r, o, 1);
        mv(nxt.paction, cur.paction, r, o, 6);
        mv(nxt.pstats, cur.pstats, r, o, 4);
        mv(nxt.phidden, cur.phidden, r, o, kHidden);
        mv(nxt.psem, cur.sem, r, o, kSensor);
        if (fixd) mv(nxt.pdepth, cur.depth, r, o, kSensor);
        src_of_[r] = o;
        obsrow_[s] = (int32_t)r;
    }
}

// the Sensor graph (sim.cpp:1183-1188; build spec DESIGN.md 3.6): every
// (agent, object, ray) through the exact predicates -- K3b
void Sim::sensor_world(uint32_t w, Table &nxt, int lo, int hi)
{
    const size_t base = (size_t)w * cap_;
    const int n = n_[w];
    if (hi < 0) hi = n;
    const bool fixd = (cfg_.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    // live food in (chunk, package) order: position and rotation
    float2 fp[kNumPkg], fr[kNumPkg];
    int nf = 0;
    for (int c = 0; c < kNumChunks; ++c) {
        const uint64_t rec = food_[(size_t)w * kNumChunks + c];
        for (int q = 0; q < kMaxPkg; ++q) {
            if (!((rec >> (40 + q)) & 1u)) continue;
            const uint32_t xy = (uint32_t)(rec >> (8 * q)) & 0xFFu;
            fp[nf] = make_float2((float)(xy & 15u) + (float)((c % kChunksX) * kChunkW),
                                 (float)(xy >> 4) + (float)((c / kChunksX) * kChunkW));
            fr[nf] = food_cs(food_rot_[((size_t)w * kMaxPkg + q) * kNumChunks + c]);
            ++nf;
        }
    }
    thread_local std::vector<float2> hd;
    hd.resize(cap_);
    // every ray's near point (nearSphere, mgr.cpp:133); the finder's at u = 0
    NearPt np[kRays];
    for (int k = 0; k < kSensor; ++k) np[k] = near_pt(ray_u(k));
    np[kSensor] = finder_np();
    for (int i = 0; i < n; ++i) heading(rw_[base + i], rz_[base + i], hd[i].x, hd[i].y);
    for (int i = lo; i < hi; ++i) {
        const float ax = x_[base + i], ay = y_[base + i];
        const float2 h = hd[i];
        // 64-bit keys in every capacity class (mbots_ray.hpp Key<>: the same
        // (depth, order) minimum as the device's 32-bit keys up to 256 slots)
        using K = uint64_t;
        K key[kRays];
        for (int k = 0; k < kRays; ++k) key[k] = Key<K>::none;
        auto fl_of = [&](float px, float py, float &f, float &l) {
            const float vx = px - ax, vy = py - ay;
            f = vx * h.x + vy * h.y;
            l = vx * h.y - vy * h.x;
        };
        for (int j = 0; j < nf; ++j) {
            float f, l;
            fl_of(fp[j].x, fp[j].y, f, l);
            const FoodBox b = box_setup(f, l, fr[j], h);
            const uint32_t order = kOrderFood + (uint32_t)j;
            for (int k = 0; k < kSensor; ++k) {
                const bool fwd = k < 24;
                if (box_hit(b, ray_u(k), fwd, np[k].c)) key[k] = std::min(key[k], Key<K>::make(box_z(b, fwd), order));
            }
            if (box_hit(b, 0.0f, true, np[kSensor].c))
                key[kSensor] = std::min(key[kSensor], Key<K>::make(box_z(b, true), order));
        }
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            float f, l;
            fl_of(x_[base + j], y_[base + j], f, l);
            const uint32_t order = kOrderAgent + (uint32_t)j;
            for (int k = 0; k < kSensor; ++k)
                key[k] = std::min(key[k], pixel_key<K>(f, l, ray_u(k), np[k], k < 24, order));
            key[kSensor] = std::min(key[kSensor], finder_key<K>(f, l, order));
        }
        // each ray's near point: in the inner rectangle (the wall is the exit
        // from it), inside a wall box (the wall, at s0) or beyond (a miss)
        auto cls_of = [&](int k, bool fwd) {
            const float ex = np[k].c * h.x + np[k].s * h.y, ey = np[k].c * h.y + np[k].s * (-h.x);
            return wall_class(fwd ? ax + ex : ax - ex, fwd ? ay + ey : ay - ey);
        };
        const size_t r = (size_t)obsrow_[base + i];
        for (int k = 0; k < kSensor; ++k) {
            const bool fwd = k < 24;
            const float u = ray_u(k), sgn = fwd ? 1.0f : -1.0f;
            const float dx = sgn * (h.x + u * h.y), dy = sgn * (h.y + u * (-h.x));
            const K kv = key[k];
            const float oz = Key<K>::z(kv);
            const uint32_t order = Key<K>::order(kv);
            const int cls = cls_of(k, fwd);
            const bool obj = (kv != Key<K>::none) && (cls == kWallInner ? beats_wall(ax, ay, dx, dy, oz) : cls == kWallNone);
            nxt.sem[r * kSensor + k] = (int8_t)(obj ? (order < kOrderAgent ? 6 : species_[base + order - kOrderAgent])
                                                    : (cls == kWallNone ? -1 : 5));
            if (fixd)
                nxt.depth[r * kSensor + k] = depth_u8(obj ? oz
                                                      : cls == kWallInner ? wall_z(ax, ay, dx, dy)
                                                      : cls == kWallBox ? np[k].c : __builtin_inff());
        }
        const K kv = key[kSensor];
        const uint32_t order = Key<K>::order(kv);
        const int fcls = cls_of(kSensor, true);
        const bool agent = kv != Key<K>::none && order >= kOrderAgent &&
                           (fcls == kWallInner ? beats_wall(ax, ay, h.x, h.y, Key<K>::z(kv)) : fcls == kWallNone);
        finder_[base + i] = agent ? (int32_t)(order - kOrderAgent) : -1;
    }
}

void Sim::arm()
{
    if (armed_) return;
    armed_ = true;
    std::fill(age_.begin(), age_.end(), (int32_t)std::min<uint64_t>(age0_, 0x7FFFFFFFu));
}

void Sim::reset_worlds(const uint32_t *global_worlds, uint32_t n, const uint32_t *episodes)
{
    arm();
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gw = global_worlds[k];
        if (gw < cfg_.world_offset || gw - cfg_.world_offset >= W_) continue;   // another rank's
        reset_flags_[gw - cfg_.world_offset] = episodes ? (int32_t)(episodes[k] + 2u) : 1;
    }
}

void Sim::set_episode_length(uint32_t steps)
{
    if (steps) arm();
    ep_len_ = steps;
}

// the reset pass of an armed Sim, before the world step (reset_worlds_kernel):
// a flagged or expired world starts over and is then stepped like the others
void Sim::reset_pass()
{
    for_worlds([&](uint32_t w) {
        const int32_t flag = reset_flags_[w], age = age_[w];
        if (flag == 0 && (ep_len_ == 0 || (uint32_t)age < ep_len_)) {
            age_[w] = age + 1;
            reset_mark_[w] = 0;
            return;
        }
        const int32_t e = flag >= 2 ? flag - 2 : episode_[w] + 1;
        init_world(w, (uint32_t)e, true);
        episode_[w] = e;
        age_[w] = 1;   // the world is stepped right after
        reset_flags_[w] = 0;
        reset_mark_[w] = 1;
    });
}

// the trajectory window's launches (traj_push_kernel, launch_traj_compute) as
// loops: the same element bodies in the same order of dependent passes
void Sim::traj_push(const TrajWin &w, uint32_t slot, const float *value) const
{
    const uint32_t N = N_, lim = std::min(N, w.max_rows);
    const Table &t = T_[tb_];
    for (uint32_t r = 0; r < lim; ++r) traj_push_row(w, slot, r, src_of_.data(), t.reward.data(), value);
    for (uint32_t k = 0; k < w.Wx * (uint32_t)kNumSpecies; ++k)
        traj_push_world(w, slot, k, N, row_base_.data(), scount_.data(), reset_mark_.data());
    w.count[slot] = N;
}

void Sim::traj_compute(const TrajWin &w, const TrajParams &P, uint32_t n)
{
    auto rows = [&](uint32_t t) { return w.count[traj_slot(w, t)]; };
    for (uint32_t t = 0; t + 1 < n; ++t)
        for (uint32_t q = 0; q < rows(t); ++q) w.next[traj_at(w, t, q)] = -1;
    for (uint32_t t = 1; t < n; ++t)
        for (uint32_t r = 0; r < rows(t); ++r) {
            const int32_t p = traj_link(w, t, r, rows(t - 1));
            if (p >= 0) w.next[traj_at(w, t - 1, (uint32_t)p)] = (int32_t)r;
        }
    for (uint32_t t = 0; t < n; ++t)
        for (uint32_t q = 0; q < rows(t); ++q) traj_sweep(w, P, n, t, q);
}

// launch_traj_sequences as loops: the starts counted per 256-row block, the
// counts scanned in (table, block) order, then each start's offset + rank
uint32_t Sim::traj_sequences(const TrajWin &w, uint32_t n, uint32_t max_count)
{
    auto rows = [&](uint32_t t) { return w.count[traj_slot(w, t)]; };
    const uint32_t bx = std::max((max_count + kTrajBlock - 1u) / kTrajBlock, 1u);
    for (uint32_t t = 0; t < n; ++t)
        for (uint32_t b = 0; b < bx; ++b) {
            uint32_t c = 0;
            for (uint32_t q = b * kTrajBlock; q < std::min(rows(t), (b + 1u) * kTrajBlock); ++q)
                c += traj_is_start(w, t, q) ? 1u : 0u;
            w.blk[t * bx + b] = c;
        }
    uint32_t S = 0;
    for (uint32_t i = 0; i < n * bx; ++i) {
        const uint32_t c = w.blk[i];
        w.blk[i] = S;
        S += c;
    }
    for (uint32_t t = 0; t < n; ++t)
        for (uint32_t b = 0; b < bx; ++b) {
            uint32_t rank = 0;
            for (uint32_t q = b * kTrajBlock; q < std::min(rows(t), (b + 1u) * kTrajBlock); ++q)
                if (traj_is_start(w, t, q)) traj_seq_walk(w, n, t, q, w.blk[t * bx + b] + rank++);
        }
    return S;
}

// launch_traj_batch as loops (o.rows / o.t0 non-null whenever obs is)
void Sim::traj_batch(const TrajWin &w, const TrajBatch &o, uint32_t lo, uint64_t B, uint32_t n, float *obs)
{
    if (B == 0) return;
    const uint64_t R = (uint64_t)n * B;
    if (o.rows) std::fill(o.rows, o.rows + R, -1);
    for (float *p : {o.reward, o.value, o.adv, o.ret})
        if (p) std::fill(p, p + R, 0.0f);
    if (o.action_in) std::fill(o.action_in, o.action_in + R, (uint8_t)0);
    for (uint32_t t = 0; t < n; ++t)
        for (uint32_t q = 0; q < w.count[traj_slot(w, t)]; ++q) traj_batch_row(w, o, lo, B, t, q);
    if (!obs) return;
    const bool depth = w.rec_bytes > 64u;
    for (uint64_t r = 0; r < R; ++r) {
        const uint8_t *rec = traj_batch_record(w, o.rows, o.t0, B, r);
        uint32_t *dst = reinterpret_cast<uint32_t *>(obs) + r * 69u;
        for (uint32_t c = 0; c < 69u; ++c) dst[c] = rec ? traj_obs_bits(rec, depth, c) : 0u;
    }
}

void Sim::traj_gather(const int32_t *rows, const int32_t *t0, uint64_t B, uint32_t n, const void *const *tables,
                      uint32_t row_bytes, void *out)
{
    const uint64_t R = (uint64_t)n * B;
    for (uint64_t o = 0; o < R; ++o) {
        char *dst = static_cast<char *>(out) + o * row_bytes;
        const int32_t q = rows[o];
        if (q < 0) memset(dst, 0, row_bytes);
        else memcpy(dst, static_cast<const char *>(tables[(uint32_t)t0[o % B] + (uint32_t)(o / B)]) + (size_t)q * row_bytes,
                    row_bytes);
    }
}

// render_kernel's images on the host: the same predicates (mbots_render.hpp),
// the agents of a row in ascending slots with the first hit final.  The image
// rows of all k images are split over the threads.
void Sim::render(const uint32_t *worlds, uint32_t k, uint32_t scale, const RenderOut &out) const
{
    const uint32_t Wp = (uint32_t)kRenderW * scale, Hp = (uint32_t)kRenderH * scale;
    const float inv = 1.0f / (float)scale;
    const uint64_t rows = (uint64_t)k * Hp;
    auto work = [&](uint64_t lo, uint64_t hi) {
        std::vector<RenderAgent> ag, hit;
        float4 food[kMaxFood];
        int nf = 0;
        uint32_t cur = 0xFFFFFFFFu;
        for (uint64_t g = lo; g < hi; ++g) {
            const uint32_t img = (uint32_t)(g / Hp), j = (uint32_t)(g % Hp);
            const uint32_t w = worlds ? worlds[img] : img;
            if (img != cur) {   // stage the image's world: its agents and live food
                cur = img;
                const size_t base = (size_t)w * cap_;
                const int n = std::min(n_[w], (int32_t)cap_);
                ag.clear();
                for (int a = 0; a < n; ++a)
                    ag.push_back(render_agent((uint32_t)a, x_[base + a], y_[base + a], rw_[base + a], rz_[base + a],
                                              species_[base + a], health_[base + a]));
                nf = 0;
                for (int c = 0; c < kNumChunks; ++c) {
                    const uint64_t rec = food_[(size_t)w * kNumChunks + c];
                    for (int q = 0; q < kMaxPkg; ++q) {
                        if (!((rec >> (40 + q)) & 1u) || nf >= kMaxFood) continue;   // (<= 30 live: stage_food)
                        const uint32_t xy = (uint32_t)(rec >> (8 * q)) & 0xFFu;
                        const float2 cs = food_cs(food_rot_[((size_t)w * kMaxPkg + q) * kNumChunks + c]);
                        food[nf++] = make_float4((float)(xy & 15u) + (float)((c % kChunksX) * kChunkW),
                                                 (float)(xy >> 4) + (float)((c / kChunksX) * kChunkW), cs.x, cs.y);
                    }
                }
            }
            const float py = render_sample(j, inv);
            hit.clear();
            for (const RenderAgent &r : ag) {
                const float dy = py - r.y;
                if (dy * dy <= kAgentR2) hit.push_back(r);
            }
            const size_t pix0 = ((size_t)img * Hp + j) * Wp;
            for (uint32_t i = 0; i < Wp; ++i) {
                const float px = render_sample(i, inv);
                uint32_t code = kRenderNoSlot;
                for (const RenderAgent &r : hit) {
                    const float dx = px - r.x, dy = py - r.y;
                    if (render_disc_hit(dx, dy * dy)) {
                        code = render_agent_code(r, dx, dy);
                        break;
                    }
                }
                if (code == kRenderNoSlot) code |= render_ground(px, py, food, nf) << 16;
                if (out.cls) out.cls[pix0 + i] = (uint8_t)render_code_cls(code);
                if (out.slot) out.slot[pix0 + i] = (int16_t)(uint16_t)(code & 0xFFFFu);
                if (out.rgb) {
                    const uint32_t c = render_code_rgb(code);
                    uint8_t *o = out.rgb + (pix0 + i) * 3;
                    o[0] = (uint8_t)c;
                    o[1] = (uint8_t)(c >> 8);
                    o[2] = (uint8_t)(c >> 16);
                }
            }
        }
    };
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(threads_, rows / 64));
    if (T == 1) return work(0, rows);
    std::vector<std::thread> th;
    th.reserve(T);
    for (unsigned t = 0; t < T; ++t) th.emplace_back(work, rows * t / T, rows * (t + 1) / T);
    for (auto &t : th) t.join();
}

void Sim::step()
{
    if (armed_) reset_pass();
    else ++age0_;
    const Table &cur = T_[tb_];
    Table &nxt = T_[tb_ ^ 1];
    for_worlds([&](uint32_t w) { world_step(w, cur); });
    scan();
    if (W_ >= 2 * threads_) {
        for_worlds([&](uint32_t w) {
            export_world(w, cur, nxt, false);
            sensor_world(w, nxt);
        });
    } else {   // few (large) worlds: the sensor split by agents over the threads
        for_worlds([&](uint32_t w) { export_world(w, cur, nxt, false); });
        sensor_by_agents(nxt);
    }
    tb_ ^= 1;
}

// the sensor over every world's agents, split evenly by agent count: each
// agent writes only its own rows and finder slot
void Sim::sensor_by_agents(Table &nxt)
{
    uint64_t G = 0;
    for (uint32_t w = 0; w < W_; ++w) G += (uint64_t)n_[w];
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(threads_, G));
    auto run = [&](uint64_t lo, uint64_t hi) {
        uint64_t g = 0;
        for (uint32_t w = 0; w < W_ && g < hi; ++w) {
            const uint64_t n = (uint64_t)n_[w];
            const uint64_t a = lo > g ? lo - g : 0, b = std::min(hi - g, n);
            if (a < b) sensor_world(w, nxt, (int)a, (int)b);
            g += n;
        }
    };
    if (T == 1) {
        run(0, G);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(T);
    for (unsigned t = 0; t < T; ++t) th.emplace_back(run, G * t / T, G * (t + 1) / T);
    for (auto &t : th) t.join();
}

// shiftObservationsSystem + shiftHiddenState (sim.cpp:1002-1048)
void Sim::shift_observations()
{
    Table &t = T_[tb_];
    const size_t n = N_;
    std::copy_n(t.species.begin(), n, t.pspecies.begin());
    std::copy_n(t.pos.begin(), 2 * n, t.ppos.begin());
    std::copy_n(t.health.begin(), n, t.phealth.begin());
    std::copy_n(t.sur.begin(), 2 * n, t.psur.begin());
    std::copy_n(t.reward.begin(), n, t.preward.begin());
    std::copy_n(t.action.begin(), 6 * n, t.paction.begin());
    for (size_t r = 0; r < n; ++r) {
        t.pstats[r * 4 + 0] = t.stats[r * 4 + 0];
        t.pstats[r * 4 + 1] = t.stats[r * 4 + 0];   // :1034 hitEnemy <- hitFriendly
        t.pstats[r * 4 + 2] = t.stats[r * 4 + 2];
        t.pstats[r * 4 + 3] = t.stats[r * 4 + 3];
    }
    std::copy_n(t.hidden.begin(), kHidden * n, t.phidden.begin());
}

void Sim::write_synthetic_actions(uint32_t seed, uint32_t step, bool write_hidden)
{
    Table &t = T_[tb_];
    for_worlds([&](uint32_t w) {
        const size_t base = (size_t)w * cap_;
        const uint32_t gw = cfg_.world_offset + w;
        for (int i = 0; i < n_[w]; ++i) {
            const size_t r = (size_t)obsrow_[base + i];
            const uint32_t k = threefry2x32(seed, step, gw, (uint32_t)i).x % 6u;
            for (uint32_t j = 0; j < 6; ++j) t.action[r * 6 + j] = j == k ? 1 : 0;
            if (write_hidden)   // both words of each draw: hidden[2k], hidden[2k + 1]
                for (int q = 0; q < kHidden / 2; ++q) {
                    const uint2 d = threefry2x32(seed ^ 0x9E3779B9u, step, gw, (uint32_t)i * (kHidden / 2) + (uint32_t)q);
                    t.hidden[r * kHidden + 2 * q] = u01(d.x) - 0.5f;
                    t.hidden[r * kHidden + 2 * q + 1] = u01(d.y) - 0.5f;
                }
        }
    });
}

void Sim::sensor_index(int32_t *out) const
{
    for (uint32_t w = 0; w < Wx_; ++w)
        for (int i = 0; i < n_[w]; ++i) out[world_off_[w] + i] = obsrow_[(size_t)w * cap_ + i];
}

uint64_t Sim::overflow() const
{
    uint64_t s = 0;
    for (uint32_t w = 0; w < Wx_; ++w) s += overflow_[w];
    return s;
}

int Sim::export_tensor(int32_t id, mbots_tensor *out)
{
    Table &t = T_[tb_];
    const bool fixd = (cfg_.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    void *p = nullptr;
    int dt = MBOTS_DTYPE_INT32;
    int64_t rows = N_, cols = 1;
    switch (id) {
    case MBOTS_EXPORT_RESET: arm(); p = reset_flags_.data(); rows = Wx_; break;   // live: whoever holds it may write
    case MBOTS_EXPORT_EPISODE: p = episode_.data(); rows = Wx_; break;
    case MBOTS_EXPORT_EPISODE_STEP:
        if (!armed_) std::fill(age_.begin(), age_.end(), (int32_t)std::min<uint64_t>(age0_, 0x7FFFFFFFu));
        p = age_.data(); rows = Wx_; break;
    case MBOTS_EXPORT_ACTION: p = t.action.data(); cols = 6; break;
    case MBOTS_EXPORT_PREV_ACTION: p = t.paction.data(); cols = 6; break;
    case MBOTS_EXPORT_HIDDEN_STATE: p = t.hidden.data(); dt = MBOTS_DTYPE_FLOAT32; cols = kHidden; break;
    case MBOTS_EXPORT_PREV_HIDDEN_STATE: p = t.phidden.data(); dt = MBOTS_DTYPE_FLOAT32; cols = kHidden; break;
    case MBOTS_EXPORT_REWARD: p = t.reward.data(); dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_PREV_REWARD: p = t.preward.data(); dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_DONE: p = zeros_rows_.data(); break;
    case MBOTS_EXPORT_POSITION: p = t.pos.data(); dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_PREV_POSITION: p = t.ppos.data(); dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_HEALTH: p = t.health.data(); dt = MBOTS_DTYPE_FLOAT32; break;   // int32 bits (B.2)
    case MBOTS_EXPORT_PREV_HEALTH: p = t.phealth.data(); dt = MBOTS_DTYPE_FLOAT32; break;
    case MBOTS_EXPORT_SURROUNDING: p = t.sur.data(); dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_PREV_SURROUNDING: p = t.psur.data(); dt = MBOTS_DTYPE_FLOAT32; cols = 2; break;
    case MBOTS_EXPORT_SENSOR_SEMANTIC: p = t.sem.data(); dt = MBOTS_DTYPE_INT8; cols = kSensor; break;
    case MBOTS_EXPORT_SENSOR_DEPTH:   // the semantic buffer unless fixed (sim.cpp:102-112, B.1)
        p = fixd ? (void *)t.depth.data() : (void *)t.sem.data(); dt = MBOTS_DTYPE_UINT8; cols = kSensor; break;
    case MBOTS_EXPORT_PREV_SENSOR_SEMANTIC: p = t.psem.data(); dt = MBOTS_DTYPE_INT8; cols = kSensor; break;
    case MBOTS_EXPORT_PREV_SENSOR_DEPTH:
        p = fixd ? (void *)t.pdepth.data() : (void *)t.psem.data(); dt = MBOTS_DTYPE_UINT8; cols = kSensor; break;
    case MBOTS_EXPORT_STATS: p = t.stats.data(); cols = 4; break;
    case MBOTS_EXPORT_PREV_STATS: p = t.pstats.data(); cols = 4; break;
    case MBOTS_EXPORT_SENSOR_INDEX: sensor_index(sensor_index_.data()); p = sensor_index_.data(); break;
    case MBOTS_EXPORT_SPECIES_COUNT: p = scount_.data(); rows = Wx_; cols = kNumSpecies; break;
    case MBOTS_EXPORT_SPECIES: p = t.species.data(); break;
    case MBOTS_EXPORT_PREV_SPECIES: p = t.pspecies.data(); break;
    default: return MBOTS_E_INVALID;
    }
    out->data = p;
    out->dtype = dt;
    out->device = -1;
    out->dims[0] = rows;
    out->dims[1] = cols;
    return MBOTS_OK;
}

// learn/util.py:14-29 over all rows: depth | health bits | position | semantic | surrounding
void Sim::construct_obs(bool prev, float *out, uint64_t out_rows) const
{
    const Table &t = T_[tb_];
    const bool fixd = (cfg_.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    const int8_t *sem = prev ? t.psem.data() : t.sem.data();
    const uint8_t *dep = fixd ? (prev ? t.pdepth.data() : t.depth.data()) : reinterpret_cast<const uint8_t *>(sem);
    const int32_t *hp = prev ? t.phealth.data() : t.health.data();
    const float *pos = prev ? t.ppos.data() : t.pos.data();
    const float *sur = prev ? t.psur.data() : t.sur.data();
    const size_t n = std::min<uint64_t>(N_, out_rows);
    for (size_t r = 0; r < n; ++r) {
        float *o = out + r * 69;
        for (int k = 0; k < kSensor; ++k) o[k] = (float)dep[r * kSensor + k];
        o[32] = u2f((uint32_t)hp[r]);
        o[33] = pos[r * 2];
        o[34] = pos[r * 2 + 1];
        for (int k = 0; k < kSensor; ++k) o[35 + k] = (float)sem[r * kSensor + k];
        o[67] = sur[r * 2];
        o[68] = sur[r * 2 + 1];
    }
}

// the device actor on host threads: the kernel's k-ordered fmaf chains, pads included
namespace {
inline void policy_layer_host(const PolLayer &L, int act, const float *in, float *out)
{
    for (uint32_t j = 0; j < L.out; ++j) {
        const float *wr = L.w + (size_t)j * L.kp;
        float acc = L.b[j];
        for (uint32_t k = 0; k < L.kp; ++k) acc = pol_fma(in[k], wr[k], acc);
        out[j] = pol_activation_any(act, acc);
    }
}
}  // namespace

void Sim::policy_segments(const PolGroups &groups, int32_t *out) const
{
    uint32_t end = 0;
    for (uint32_t s = 0; s < (uint32_t)kNumSpecies; ++s) {
        end += totals_[1 + s];
        for (uint32_t g = 0; g < groups.G; ++g) {
            int32_t *o = out + 2u * (4u * g + s);
            o[0] = (int32_t)pol_group_edge(row_base_.data(), Wx_, groups.first[g], s, end);
            o[1] = (int32_t)pol_group_edge(row_base_.data(), Wx_, groups.first[g + 1u], s, end);
        }
    }
}

void Sim::policy_act(const PolGroups &groups, uint32_t flags, uint32_t draw, int32_t *action_out, float *logp_out,
                     float *value_out, uint64_t out_rows)
{
    Table &t = T_[tb_];
    const bool fixd = (cfg_.flags & MBOTS_FLAG_FIX_DEPTH_ALIAS) != 0;
    const uint8_t *dep = fixd ? t.depth.data() : reinterpret_cast<const uint8_t *>(t.sem.data());
    const bool write = !(flags & kActNoWrite), greedy = (flags & kActGreedy) != 0;
    for_worlds([&](uint32_t w) {
        float a[kPolMaxH + 4], b[kPolMaxH + 4], hid[kPolMaxH], z[16], v[1], mem[kHidden], gate[kHidden];
        uint32_t g = groups.ghost;   // the world's group: the ghost's, or the one whose local range holds w
        if (w < Wx_)
            for (g = 0; groups.first[g + 1u] <= w; ++g) {}
        for (int s = 0; s < kNumSpecies; ++s) {
            const PolNet &net = groups.table[4u * g + (uint32_t)s];
            const int32_t base = row_base_[(size_t)w * kNumSpecies + s], cnt = scount_[(size_t)w * kNumSpecies + s];
            for (int32_t k = 0; k < cnt; ++k) {
                const size_t r = (size_t)(base + k);
                pol_row_input(a, dep + r * kSensor, t.sem.data() + r * kSensor, t.health[r], &t.pos[r * 2],
                              &t.sur[r * 2], (net.flags & kPolMemoryIn) ? &t.hidden[r * kHidden] : nullptr,
                              net.trunk[0].kp);
                float *cur = a, *oth = b;
                for (uint32_t l = 0; l < net.n_trunk; ++l) {
                    policy_layer_host(net.trunk[l], (int)net.trunk[l].act, cur, oth);
                    std::swap(cur, oth);
                }
                policy_layer_host(net.actor[0], kActRelu, cur, hid);
                policy_layer_host(net.actor[1], kActIdentity, hid, z);
                policy_layer_host(net.critic[0], kActRelu, cur, hid);
                policy_layer_host(net.critic[1], kActIdentity, hid, v);
                if (net.has_memory) policy_layer_host(net.memory, kActTanh, cur, mem);
                if (net.gated) {   // the blend with the HiddenState the row read
                    policy_layer_host(net.gate, kActSigmoid, cur, gate);
                    for (int i = 0; i < kHidden; ++i) mem[i] = pol_gate_blend(gate[i], mem[i], t.hidden[r * kHidden + i]);
                }
                const float u = pol_uniform(cfg_.rand_seed, draw, cfg_.world_offset + w, (uint32_t)s + 1u, (uint32_t)k);
                float logp;
                const int32_t act = pol_sample(z, u, greedy, &logp);
                if (write) {
                    for (int i = 0; i < kPolActions; ++i) t.action[r * 6 + i] = act == i ? 1 : 0;
                    if (net.has_memory)
                        for (int i = 0; i < kHidden; ++i) t.hidden[r * kHidden + i] = mem[i];
                }
                if (r < out_rows) {
                    if (action_out) action_out[r] = act;
                    if (logp_out) logp_out[r] = logp;
                    if (value_out) value_out[r] = v[0];
                }
            }
        }
    });
}

// ---- evaluate and its backward pass (DESIGN.md "Differentiable evaluate") ----
namespace {
unsigned host_threads()
{
    const char *e = getenv("MBOTS_CPU_THREADS");
    const unsigned n = e ? (unsigned)atoi(e) : std::min(16u, std::thread::hardware_concurrency());
    return n ? n : 1u;
}

// fn(i) for i in [0, n) on contiguous ranges over the host threads
template <typename F> void par_for(uint64_t n, uint64_t grain, F &&fn)
{
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(host_threads(), n / std::max<uint64_t>(grain, 1)));
    if (T == 1) {
        for (uint64_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(T);
    for (unsigned t = 0; t < T; ++t) {
        const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
        th.emplace_back([&fn, lo, hi] {
            for (uint64_t i = lo; i < hi; ++i) fn(i);
        });
    }
    for (auto &t : th) t.join();
}

// one row's forward with every layer's output kept: y[0] the padded input,
// y[l + 1] trunk layer l's output
struct RowForward {
    float y[kPolMaxTrunk + 1][kPolMaxH + 4], ha[kPolMaxH], hc[kPolMaxH], z[16], v[1];
};

void row_forward(const PolNet &net, const float *o, const float *hidden, RowForward &f)
{
    float *x = f.y[0];
    for (int k = 0; k < kPolObs; ++k) x[k] = o[k];
    uint32_t n = kPolObs;
    if (net.flags & kPolMemoryIn)
        for (int k = 0; k < kHidden; ++k) x[n++] = hidden[k];
    while (n < net.trunk[0].kp) x[n++] = 0.0f;
    for (uint32_t l = 0; l < net.n_trunk; ++l) policy_layer_host(net.trunk[l], (int)net.trunk[l].act, f.y[l], f.y[l + 1]);
    const float *top = f.y[net.n_trunk];
    policy_layer_host(net.actor[0], kActRelu, top, f.ha);
    policy_layer_host(net.actor[1], kActIdentity, f.ha, f.z);
    policy_layer_host(net.critic[0], kActRelu, top, f.hc);
    policy_layer_host(net.critic[1], kActIdentity, f.hc, f.v);
}
void row_forward(const PolNet &net, const PolEvalIO &io, uint64_t r, RowForward &f)
{
    row_forward(net, io.obs + r * kPolObs, io.hidden ? io.hidden + r * kHidden : nullptr, f);
}

// the layer's chains continued by one row: db[j] + d[j], fmaf(d[j], x[k], dW[j][k])
inline void grad_w_row(const PolLayer &L, const float *d, const float *x, float *sw, float *sb)
{
    for (uint32_t j = 0; j < L.out; ++j) {
        const float dj = d[j];
        sb[j] = sb[j] + dj;
        float *w = sw + (size_t)j * L.in;
        for (uint32_t k = 0; k < L.in; ++k) w[k] = pol_fma(dj, x[k], w[k]);
    }
}
// the layer's input gradient: g[k] = sum over j ascending of fmaf(d[j], W[j][k], .), from +0
inline void grad_x_row(const PolLayer &L, const float *d, float *g)
{
    for (uint32_t k = 0; k < L.in; ++k) g[k] = 0.0f;
    for (uint32_t j = 0; j < L.out; ++j) {
        const float dj = d[j];
        const float *w = L.w + (size_t)j * L.kp;
        for (uint32_t k = 0; k < L.in; ++k) g[k] = pol_fma(dj, w[k], g[k]);
    }
}
}  // namespace

// the accumulators added in ascending index
static void policy_grad_reduce(const PolGradSlabs &S, const PolGradOut &out)
{
    for (uint32_t l = 0; l < out.n; ++l) {
        const uint64_t nw = out.w[l] ? (uint64_t)out.in[l] * out.out[l] : 0u, nb = out.b[l] ? out.out[l] : 0u;
        par_for(nw + nb, 4096, [&](uint64_t i) {
            const size_t off = i < nw ? S.w[l] + i : S.b[l] + (i - nw);
            float acc = 0.0f;
            for (uint32_t a = 0; a < S.nacc; ++a) acc = acc + S.base[(size_t)a * S.slab_floats + off];
            if (i < nw) out.w[l][i] = acc;
            else out.b[l][i - nw] = acc;
        });
    }
}

void policy_eval(const PolNet &net, const PolEvalIO &io)
{
    par_for(io.n, 64, [&](uint64_t r) {
        RowForward f;
        row_forward(net, io, r, f);
        float logp, ent, dz[kPolActions];
        pol_head(f.z, io.action[r], 0.0f, 0.0f, &logp, &ent, dz);
        if (io.logp) io.logp[r] = logp;
        if (io.value) io.value[r] = f.v[0];
        if (io.entropy) io.entropy[r] = ent;
    });
}

void policy_grad(const PolNet &net, const PolEvalIO &io, const PolGradSlabs &S, const PolGradOut &out)
{
    const uint64_t tiles = (io.n + kPolGradRows - 1u) / kPolGradRows;
    const uint32_t T = net.n_trunk;
    par_for(S.nacc, 1, [&](uint64_t a) {
        float *slab = S.base + a * S.slab_floats;
        std::fill(slab, slab + S.slab_floats, 0.0f);
        RowForward f;
        float d0[kPolMaxH], d1[kPolMaxH], ga[kPolMaxH], gc[kPolMaxH];
        for (uint64_t tile = a; tile < tiles; tile += kPolGradAcc) {
            const uint64_t r1 = std::min<uint64_t>(io.n, (tile + 1u) * kPolGradRows);
            for (uint64_t r = tile * kPolGradRows; r < r1; ++r) {
                row_forward(net, io, r, f);
                float logp, ent, dz[kPolActions];
                pol_head(f.z, io.action[r], io.g_logp ? io.g_logp[r] : 0.0f, io.g_entropy ? io.g_entropy[r] : 0.0f, &logp,
                         &ent, dz);
                const float dv[1] = {io.g_value ? io.g_value[r] : 0.0f};
                const float *top = f.y[T];
                // heads: second layers, then the hidden layers' gradients in place of ReLU's outputs
                grad_w_row(net.actor[1], dz, f.ha, slab + S.w[kPolMaxTrunk + 1], slab + S.b[kPolMaxTrunk + 1]);
                grad_w_row(net.critic[1], dv, f.hc, slab + S.w[kPolMaxTrunk + 3], slab + S.b[kPolMaxTrunk + 3]);
                grad_x_row(net.actor[1], dz, d0);
                grad_x_row(net.critic[1], dv, d1);
                for (uint32_t k = 0; k < net.H; ++k) {
                    d0[k] = d0[k] * pol_activation_grad(kActRelu, f.ha[k]);
                    d1[k] = d1[k] * pol_activation_grad(kActRelu, f.hc[k]);
                }
                grad_w_row(net.actor[0], d0, top, slab + S.w[kPolMaxTrunk], slab + S.b[kPolMaxTrunk]);
                grad_w_row(net.critic[0], d1, top, slab + S.w[kPolMaxTrunk + 2], slab + S.b[kPolMaxTrunk + 2]);
                grad_x_row(net.actor[0], d0, ga);
                grad_x_row(net.critic[0], d1, gc);
                float *d = d0, *g = d1;
                for (uint32_t k = 0; k < net.H; ++k)
                    d[k] = (ga[k] + gc[k]) * pol_activation_grad((int)net.trunk[T - 1u].act, top[k]);
                for (uint32_t l = T; l-- > 0u;) {
                    grad_w_row(net.trunk[l], d, f.y[l], slab + S.w[l], slab + S.b[l]);
                    if (l == 0u) break;
                    grad_x_row(net.trunk[l], d, g);
                    for (uint32_t k = 0; k < net.H; ++k)
                        g[k] = g[k] * pol_activation_grad((int)net.trunk[l - 1u].act, f.y[l][k]);
                    std::swap(d, g);
                }
            }
        }
    });
    policy_grad_reduce(S, out);
}

// ---- evaluate_sequences (DESIGN.md "Backpropagation through HiddenState") ----
namespace {
inline uint32_t seq_len(const PolSeqIO &io, uint64_t b)
{
    const int32_t n = io.length[b];
    return n < 0 ? 0u : std::min((uint32_t)n, io.L);
}
// the batch column position p of a call stands for, and the positions it runs
inline uint64_t seq_col(const PolSeqCols &cols, uint64_t p) { return cols.idx ? (uint64_t)cols.idx[p] : p; }
inline uint64_t seq_cols(const PolSeqCols &cols, const PolSeqIO &io) { return cols.idx ? cols.n : io.B; }
// h_{k+1} from the trunk's last output and h_k: the memory head's output, a
// gated net's blended with h_k (out may be h)
inline void seq_next_h(const PolNet &net, const float *top, const float *h, float *out)
{
    float c[kHidden], z[kHidden];
    policy_layer_host(net.memory, kActTanh, top, c);
    if (net.gated) {
        policy_layer_host(net.gate, kActSigmoid, top, z);
        for (int i = 0; i < kHidden; ++i) c[i] = pol_gate_blend(z[i], c[i], h[i]);
    }
    for (int i = 0; i < kHidden; ++i) out[i] = c[i];
}
}  // namespace

void policy_seq_eval(const PolNet &net, const PolSeqIO &io, const PolSeqCols &cols)
{
    par_for(seq_cols(cols, io), 16, [&](uint64_t p) {
        const uint64_t b = seq_col(cols, p);
        RowForward f;
        float h[kHidden], y[kHidden];
        for (int c = 0; c < kHidden; ++c) h[c] = io.hidden0[b * kHidden + c];
        const uint32_t n = seq_len(io, b);
        for (uint32_t k = 0; k < io.L; ++k) {
            const uint64_t e = (uint64_t)k * io.B + b;
            if (k >= n) {
                if (io.logp) io.logp[e] = 0.0f;
                if (io.value) io.value[e] = 0.0f;
                if (io.entropy) io.entropy[e] = 0.0f;
                if (io.hidden)
                    for (int c = 0; c < kHidden; ++c) io.hidden[e * kHidden + c] = 0.0f;
                continue;
            }
            row_forward(net, io.obs + e * kPolObs, h, f);
            seq_next_h(net, f.y[net.n_trunk], h, y);
            float logp, ent, dz[kPolActions];
            pol_head(f.z, io.action[e], 0.0f, 0.0f, &logp, &ent, dz);
            if (io.logp) io.logp[e] = logp;
            if (io.value) io.value[e] = f.v[0];
            if (io.entropy) io.entropy[e] = ent;
            if (io.hidden)
                for (int c = 0; c < kHidden; ++c) io.hidden[e * kHidden + c] = h[c];
            for (int c = 0; c < kHidden; ++c) h[c] = y[c];
        }
    });
}

void policy_seq_grad(const PolNet &net, const PolSeqIO &io, const PolGradSlabs &S, float *hws, const PolGradOut &out,
                     const PolSeqCols &cols)
{
    const uint64_t ncols = seq_cols(cols, io);
    const uint64_t tiles = (ncols + kPolGradRows - 1u) / kPolGradRows;
    const uint32_t T = net.n_trunk;
    constexpr int kM = kPolGradLayers;   // the memory head's slot
    constexpr int kG = kPolSeqLayers;    // the gate head's
    par_for(S.nacc, 1, [&](uint64_t a) {
        float *slab = S.base + a * S.slab_floats;
        std::fill(slab, slab + S.slab_floats, 0.0f);
        float *hk = hws + a * (size_t)io.L * kPolGradRows * kHidden;   // [L][64][16]
        RowForward f;
        float d0[kPolMaxH], d1[kPolMaxH], ga[kPolMaxH], gc[kPolMaxH], gm[kPolMaxH], gg[kPolMaxH], y[kHidden], dm[kHidden],
            zg[kHidden], dg[kHidden], dd[kHidden];
        float dh[kPolGradRows][kHidden];
        for (uint64_t tile = a; tile < tiles; tile += kPolGradAcc) {
            const uint64_t b0 = tile * kPolGradRows;
            const uint32_t nb = (uint32_t)std::min<uint64_t>(kPolGradRows, ncols - b0);
            // the forward sweep: every present element's h_k
            uint32_t maxlen = 0;
            for (uint32_t r = 0; r < nb; ++r) {
                const uint64_t b = seq_col(cols, b0 + r);
                const uint32_t n = seq_len(io, b);
                maxlen = std::max(maxlen, n);
                float h[kHidden];
                for (int c = 0; c < kHidden; ++c) h[c] = io.hidden0[b * kHidden + c];
                for (uint32_t k = 0; k < n; ++k) {
                    float *o = hk + ((size_t)k * kPolGradRows + r) * kHidden;
                    for (int c = 0; c < kHidden; ++c) o[c] = h[c];
                    if (k + 1u == n) break;
                    row_forward(net, io.obs + ((uint64_t)k * io.B + b) * kPolObs, h, f);
                    seq_next_h(net, f.y[T], h, h);
                }
                for (int c = 0; c < kHidden; ++c) dh[r][c] = 0.0f;
            }
            // backward in time.  (An absent element is a row of +0 inputs and
            // gradients: it leaves every chain as it is, and is skipped.)
            for (uint32_t k = maxlen; k-- > 0u;)
                for (uint32_t r = 0; r < nb; ++r) {
                    const uint64_t b = seq_col(cols, b0 + r);
                    if (k >= seq_len(io, b)) continue;
                    const uint64_t e = (uint64_t)k * io.B + b;
                    const float *hcur = hk + ((size_t)k * kPolGradRows + r) * kHidden;
                    row_forward(net, io.obs + e * kPolObs, hcur, f);
                    const float *top = f.y[T];
                    policy_layer_host(net.memory, kActTanh, top, y);
                    float logp, ent, dz[kPolActions];
                    pol_head(f.z, io.action[e], io.g_logp ? io.g_logp[e] : 0.0f, io.g_entropy ? io.g_entropy[e] : 0.0f,
                             &logp, &ent, dz);
                    const float dv[1] = {io.g_value ? io.g_value[e] : 0.0f};
                    if (!net.gated) {
                        for (int c = 0; c < kHidden; ++c) dm[c] = dh[r][c] * pol_activation_grad(kActTanh, y[c]);
                    } else {
                        policy_layer_host(net.gate, kActSigmoid, top, zg);
                        for (int c = 0; c < kHidden; ++c) pol_gate_back(dh[r][c], zg[c], y[c], hcur[c], &dm[c], &dg[c], &dd[c]);
                    }
                    grad_w_row(net.actor[1], dz, f.ha, slab + S.w[kPolMaxTrunk + 1], slab + S.b[kPolMaxTrunk + 1]);
                    grad_w_row(net.critic[1], dv, f.hc, slab + S.w[kPolMaxTrunk + 3], slab + S.b[kPolMaxTrunk + 3]);
                    grad_w_row(net.memory, dm, top, slab + S.w[kM], slab + S.b[kM]);
                    if (net.gated) grad_w_row(net.gate, dg, top, slab + S.w[kG], slab + S.b[kG]);
                    grad_x_row(net.actor[1], dz, d0);
                    grad_x_row(net.critic[1], dv, d1);
                    for (uint32_t j = 0; j < net.H; ++j) {
                        d0[j] = d0[j] * pol_activation_grad(kActRelu, f.ha[j]);
                        d1[j] = d1[j] * pol_activation_grad(kActRelu, f.hc[j]);
                    }
                    grad_w_row(net.actor[0], d0, top, slab + S.w[kPolMaxTrunk], slab + S.b[kPolMaxTrunk]);
                    grad_w_row(net.critic[0], d1, top, slab + S.w[kPolMaxTrunk + 2], slab + S.b[kPolMaxTrunk + 2]);
                    grad_x_row(net.actor[0], d0, ga);
                    grad_x_row(net.critic[0], d1, gc);
                    grad_x_row(net.memory, dm, gm);
                    if (net.gated) grad_x_row(net.gate, dg, gg);
                    float *d = d0, *g = d1;
                    for (uint32_t j = 0; j < net.H; ++j) {
                        float in = (ga[j] + gc[j]) + gm[j];
                        if (net.gated) in = in + gg[j];
                        d[j] = in * pol_activation_grad((int)net.trunk[T - 1u].act, top[j]);
                    }
                    for (uint32_t l = T; l-- > 0u;) {
                        grad_w_row(net.trunk[l], d, f.y[l], slab + S.w[l], slab + S.b[l]);
                        if (l == 0u) break;
                        grad_x_row(net.trunk[l], d, g);
                        for (uint32_t j = 0; j < net.H; ++j)
                            g[j] = g[j] * pol_activation_grad((int)net.trunk[l - 1u].act, f.y[l][j]);
                        std::swap(d, g);
                    }
                    // dh_k from the first layer's HiddenState columns
                    for (int c = 0; c < kHidden; ++c) {
                        float acc = 0.0f;
                        for (uint32_t j = 0; j < net.H; ++j)
                            acc = pol_fma(d[j], net.trunk[0].w[(size_t)j * net.trunk[0].kp + kPolObs + c], acc);
                        dh[r][c] = net.gated ? dd[c] + acc : acc;
                    }
                }
        }
    });
    policy_grad_reduce(S, out);
}

void Sim::world_state(uint32_t w, float *xy_rwrz, int32_t *sp_hp_finder, uint64_t *food,
                      uint32_t *food_rot, int32_t *n_out) const
{
    const size_t base = (size_t)w * cap_;
    for (uint32_t i = 0; i < cap_; ++i) {
        xy_rwrz[i * 4 + 0] = x_[base + i];
        xy_rwrz[i * 4 + 1] = y_[base + i];
        xy_rwrz[i * 4 + 2] = rw_[base + i];
        xy_rwrz[i * 4 + 3] = rz_[base + i];
        sp_hp_finder[i * 3 + 0] = species_[base + i];
        sp_hp_finder[i * 3 + 1] = health_[base + i];
        sp_hp_finder[i * 3 + 2] = finder_[base + i];
    }
    memcpy(food, &food_[(size_t)w * kNumChunks], kNumChunks * sizeof(uint64_t));
    if (food_rot) memcpy(food_rot, &food_rot_[(size_t)w * kNumPkg], kNumPkg * sizeof(uint32_t));
    *n_out = n_[w];
}

void Sim::set_world_state(uint32_t w, const float *xy_rwrz, const uint64_t *food, const uint32_t *food_rot,
                          int32_t n_food)
{
    const size_t base = (size_t)w * cap_;
    for (int32_t i = 0; i < n_[w]; ++i) {
        x_[base + i] = xy_rwrz[i * 4 + 0];
        y_[base + i] = xy_rwrz[i * 4 + 1];
        rw_[base + i] = xy_rwrz[i * 4 + 2];
        rz_[base + i] = xy_rwrz[i * 4 + 3];
    }
    memcpy(&food_[(size_t)w * kNumChunks], food, kNumChunks * sizeof(uint64_t));
    memcpy(&food_rot_[(size_t)w * kNumPkg], food_rot, kNumPkg * sizeof(uint32_t));
    cur_food_[w] = n_food;
}

// ---- checkpoint: the config, every state array and the live table half ----
namespace {
constexpr char kMagic[8] = {'M', 'B', 'O', 'T', 'S', 'C', 'P', 'U'};
}  // namespace

#define MB_CPU_SLOT_ARRAYS(X)                                                                     \
    X(x_) X(y_) X(rw_) X(rz_) X(sur0_) X(sur1_) X(species_) X(health_) X(finder_) X(obsrow_)       \
    X(stats_)
#define MB_CPU_WORLD_ARRAYS(X)                                                                    \
    X(n_) X(cur_food_) X(scount_) X(row_base_) X(world_off_) X(key_) X(ctr_) X(overflow_)         \
    X(food_rot_) X(food_) X(sreward_)
#define MB_CPU_ARRAYS(X) MB_CPU_SLOT_ARRAYS(X) MB_CPU_WORLD_ARRAYS(X)
#define MB_CPU_TABLE(X)                                                                           \
    X(species) X(health) X(action) X(stats) X(pspecies) X(phealth) X(paction) X(pstats) X(pos)     \
    X(sur) X(reward) X(hidden) X(ppos) X(psur) X(preward) X(phidden) X(sem) X(psem) X(depth)      \
    X(pdepth)

// an armed Sim's blob ends with a trailer (an unarmed one's is what it always
// was): magic, the episode length, then episode, age and the pending flags per
// simulated world
namespace {
constexpr char kEpMagic[8] = {'M', 'B', 'O', 'T', 'S', 'E', 'P', '5'};
}  // namespace

uint64_t Sim::checkpoint_bytes() const
{
    uint64_t b = armed_ ? sizeof(kEpMagic) + 4 + (uint64_t)W_ * 12 : 0;
    b += sizeof(kMagic) + sizeof(mbots_config) + sizeof(N_) + sizeof(totals_) + sizeof(agent_steps_);
#define X(v) b += v.size() * sizeof(v[0]);
    MB_CPU_ARRAYS(X)
#undef X
    const Table &t = T_[tb_];
#define X(c) b += t.c.size() * sizeof(t.c[0]);
    MB_CPU_TABLE(X)
#undef X
    return b;
}

int Sim::save(void *dst, uint64_t bytes, std::string &err) const
{
    if (bytes < checkpoint_bytes()) { err = "checkpoint buffer too small"; return MBOTS_E_INVALID; }
    char *p = static_cast<char *>(dst);
    auto w = [&](const void *s, size_t n) { memcpy(p, s, n); p += n; };
    w(kMagic, sizeof(kMagic));
    w(&cfg_, sizeof(cfg_));
    w(&N_, sizeof(N_));
    w(totals_, sizeof(totals_));
    w(&agent_steps_, sizeof(agent_steps_));
#define X(v) w(v.data(), v.size() * sizeof(v[0]));
    MB_CPU_ARRAYS(X)
#undef X
    const Table &t = T_[tb_];
#define X(c) w(t.c.data(), t.c.size() * sizeof(t.c[0]));
    MB_CPU_TABLE(X)
#undef X
    if (armed_) {
        w(kEpMagic, sizeof(kEpMagic));
        w(&ep_len_, 4);
        w(episode_.data(), (size_t)W_ * 4);
        w(age_.data(), (size_t)W_ * 4);
        w(reset_flags_.data(), (size_t)W_ * 4);
    }
    return MBOTS_OK;
}

int Sim::load(const void *src, uint64_t bytes, std::string &err)
{
    if (bytes < sizeof(kMagic) + sizeof(mbots_config)) { err = "checkpoint truncated"; return MBOTS_E_INVALID; }
    const char *p = static_cast<const char *>(src);
    if (memcmp(p, kMagic, sizeof(kMagic)) != 0) { err = "not a CPU-mode checkpoint"; return MBOTS_E_INVALID; }
    mbots_config c;
    memcpy(&c, p + sizeof(kMagic), sizeof(c));
    // (another agent_capacity is fine when every world of the blob fits this
    // one's: the per-slot arrays are re-laid out world by world, the table's
    // first N rows copied -- SimManager(agent_capacity="auto"))
    if (c.num_worlds != cfg_.num_worlds || c.agent_capacity < 4 || c.agent_capacity > (uint32_t)kMaxCap ||
        c.init_num_agents_per_world != cfg_.init_num_agents_per_world ||
        c.world_offset != cfg_.world_offset || c.flags != cfg_.flags || c.rand_seed != cfg_.rand_seed) {
        err = "checkpoint configuration differs from the manager's";
        return MBOTS_E_INVALID;
    }
    const size_t cap_src = c.agent_capacity;
    // bytes of array v in the blob: per-slot arrays and table columns scale
    // with the capacity, per-world arrays do not
    auto src_bytes = [&](size_t elems, size_t elem_bytes, bool per_slot) {
        return (per_slot ? elems / cap_ * cap_src : elems) * elem_bytes;
    };
    size_t need = sizeof(kMagic) + sizeof(mbots_config) + sizeof(N_) + sizeof(totals_) + sizeof(agent_steps_);
    size_t n_off = 0;
#define X(v) need += src_bytes(v.size(), sizeof(v[0]), true);
    MB_CPU_SLOT_ARRAYS(X)
#undef X
    n_off = need;
#define X(v) need += src_bytes(v.size(), sizeof(v[0]), false);
    MB_CPU_WORLD_ARRAYS(X)
#undef X
    const Table &t0 = T_[0];
#define X(c) need += src_bytes(t0.c.size(), sizeof(t0.c[0]), true);
    MB_CPU_TABLE(X)
#undef X
    const size_t trailer = sizeof(kEpMagic) + 4 + (size_t)W_ * 12;
    const bool episodes = bytes == need + trailer && memcmp(p + need, kEpMagic, sizeof(kEpMagic)) == 0;
    if (bytes != need && !episodes) { err = "checkpoint size mismatch"; return MBOTS_E_INVALID; }
    for (uint32_t w = 0; w < W_; ++w) {   // n_ leads the per-world arrays
        int32_t n;
        memcpy(&n, p + n_off + 4 * (size_t)w, 4);
        if (n < 0 || (size_t)n > cap_) {
            err = "a world of the checkpoint holds " + std::to_string(n) + " agents, more than agent_capacity " +
                  std::to_string(cap_);
            return MBOTS_E_INVALID;
        }
    }
    p += sizeof(kMagic) + sizeof(c);
    auto r = [&](void *d, size_t n) { memcpy(d, p, n); p += n; };
    r(&N_, sizeof(N_));
    r(totals_, sizeof(totals_));
    r(&agent_steps_, sizeof(agent_steps_));
    auto slot = [&](auto &v) {   // [world][cap_src] -> [world][cap_]
        using E = std::remove_reference_t<decltype(v[0])>;
        const size_t keep = std::min(cap_src, (size_t)cap_);
        for (size_t w = 0; w < v.size() / cap_; ++w) memcpy(&v[w * cap_], p + w * cap_src * sizeof(E), keep * sizeof(E));
        p += v.size() / cap_ * cap_src * sizeof(E);
    };
#define X(v) slot(v);
    MB_CPU_SLOT_ARRAYS(X)
#undef X
#define X(v) r(v.data(), v.size() * sizeof(v[0]));
    MB_CPU_WORLD_ARRAYS(X)
#undef X
    tb_ = 0;
    Table &t = T_[0];
    auto col = [&](auto &v) {   // the first N rows live; the rest stale
        using E = std::remove_reference_t<decltype(v[0])>;
        const size_t sb = v.size() / cap_ * cap_src * sizeof(E);
        memcpy(v.data(), p, std::min(sb, v.size() * sizeof(E)));
        p += sb;
    };
#define X(c) col(t.c);
    MB_CPU_TABLE(X)
#undef X
    // episodes: an armed Sim's blob brings its armed state along; an unarmed
    // one's knows no episodes -- an armed Sim stays armed, keeps its episode
    // length and starts every world at episode 0, age 0, no flag pending
    if (episodes) {
        p += sizeof(kEpMagic);
        armed_ = true;
        r(&ep_len_, 4);
        r(episode_.data(), (size_t)W_ * 4);
        r(age_.data(), (size_t)W_ * 4);
        r(reset_flags_.data(), (size_t)W_ * 4);
    } else {
        std::fill(episode_.begin(), episode_.end(), 0);
        std::fill(age_.begin(), age_.end(), 0);
        std::fill(reset_flags_.begin(), reset_flags_.end(), 0);
        age0_ = 0;
    }
    return MBOTS_OK;
}

int Sim::grow(uint32_t new_cap, std::string &err)
{
    const size_t rows_old = (size_t)W_ * cap_, rows = (size_t)W_ * new_cap;
    try {
        // everything new first: a failed allocation leaves the Sim as it was
        auto slots = [&](const auto &v) {   // [world][cap_] -> [world][new_cap], the new slots zero
            std::remove_const_t<std::remove_reference_t<decltype(v)>> o(rows);
            for (size_t w = 0; w < W_; ++w) std::copy_n(v.begin() + w * cap_, cap_, o.begin() + w * new_cap);
            return o;
        };
#define X(v) auto n##v = slots(v);
        MB_CPU_SLOT_ARRAYS(X)
#undef X
        Table t0, t1;
        t0.resize(rows);
        t1.resize(rows);
        const Table &cur = T_[tb_];
#define X(c) std::copy_n(cur.c.begin(), cur.c.size(), t0.c.begin());
        MB_CPU_TABLE(X)
#undef X
        std::vector<int32_t> zr(rows), si(rows), so(rows);
        std::copy_n(src_of_.begin(), rows_old, so.begin());
        struct Retired {
            Table t[2];
            std::vector<int32_t> zeros_rows, sensor_index;
        };
        auto old = std::make_shared<Retired>();
        retired_.reserve(retired_.size() + 1);
        // from here on only moves: nothing throws (the buffers, and views of
        // them, stay where they are)
        old->t[0] = std::move(T_[0]);
        old->t[1] = std::move(T_[1]);
        old->zeros_rows = std::move(zeros_rows_);
        old->sensor_index = std::move(sensor_index_);
        retired_.push_back(std::move(old));
#define X(v) v = std::move(n##v);
        MB_CPU_SLOT_ARRAYS(X)
#undef X
        T_[0] = std::move(t0);
        T_[1] = std::move(t1);
        zeros_rows_ = std::move(zr);
        sensor_index_ = std::move(si);
        src_of_ = std::move(so);
    } catch (const std::bad_alloc &) {
        err = "host allocation for agent_capacity " + std::to_string(new_cap) + " failed";
        return MBOTS_E_NOMEM;
    }
    tb_ = 0;
    cap_ = new_cap;
    cfg_.agent_capacity = new_cap;
    return MBOTS_OK;
}

}  // namespace cpu
}  // namespace mbots
