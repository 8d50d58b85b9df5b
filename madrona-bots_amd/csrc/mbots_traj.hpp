// mbots_traj.hpp -- the trajectory window (include/mbots.h "Trajectory
// window"): its storage descriptor and the per-element bodies of the push, the
// `next` inversion and the sweep, shared by the HIP kernels
// (mbots_kernels.hip) and the CPU mode's loops (mbots_cpu.cpp) so that both
// give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mbots {

constexpr int kTrajEndNone = 0, kTrajEndDied = 1, kTrajEndReset = 2, kTrajEndWindow = 3;

// A window of `horizon` table slots of `max_rows` rows each (device memory, or
// host memory in CPU mode).  The slots are a ring: table t of the window lives
// in slot (base + t) % horizon, so clear(keep_last) moves no data.
struct TrajWin {
    int32_t *link, *world, *next, *end;     // [horizon][max_rows]
    float *reward, *value, *adv, *ret;      // [horizon][max_rows]
    int32_t *mark;                          // [horizon][Wx]: world re-initialised by the table's step
    uint32_t *count;                        // [horizon]: N_t as pushed (may exceed max_rows: the
                                            // table is then truncated and compute refuses it)
    uint32_t horizon, max_rows, Wx, world_offset;
    uint32_t base;                          // slot of table 0
};

__host__ __device__ inline uint32_t traj_slot(const TrajWin &w, uint32_t t) { return (w.base + t) % w.horizon; }
__host__ __device__ inline size_t traj_at(const TrajWin &w, uint32_t t, uint32_t r)
{
    return (size_t)traj_slot(w, t) * w.max_rows + r;
}

// every product and every sum of the sweep rounded to f32 on its own
__host__ __device__ inline float traj_mul(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fmul_rn(a, b);
#else
    volatile float p = a * b;   // (the library is built without contraction; this keeps it so)
    return p;
#endif
}
__host__ __device__ inline float traj_add(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fadd_rn(a, b);
#else
    volatile float s = a + b;
    return s;
#endif
}

// push, row part: row r < min(N, max_rows) of the current table into slot s
__host__ __device__ inline void traj_push_row(const TrajWin &w, uint32_t s, uint32_t r, const int32_t *src_of,
                                              const float *reward, const float *value)
{
    const size_t i = (size_t)s * w.max_rows + r;
    w.link[i] = src_of[r];
    w.reward[i] = reward[r];
    w.value[i] = value ? value[r] : 0.0f;
}
// push, world part: item k = species * Wx + world of the exported worlds (the
// table's own order: consecutive items own consecutive rows) fills its rows'
// world index (row_base / scount: K2's row bases and K1's species counts of the
// table, both [world][4]); the first species' item also copies the world's
// reset mark
__host__ __device__ inline void traj_push_world(const TrajWin &w, uint32_t s, uint32_t k, uint32_t N,
                                                const int32_t *row_base, const int32_t *scount,
                                                const int32_t *reset_mark)
{
    const uint32_t wl = k % w.Wx, sp = k / w.Wx;
    const int32_t b = row_base[4u * wl + sp], c = scount[4u * wl + sp];
    const uint32_t lim = N < w.max_rows ? N : w.max_rows;
    for (int32_t j = 0; j < c; ++j) {
        const uint32_t r = (uint32_t)(b + j);
        if (r < lim) w.world[(size_t)s * w.max_rows + r] = (int32_t)(w.world_offset + wl);
    }
    if (sp == 0u) w.mark[(size_t)s * w.Wx + wl] = reset_mark ? reset_mark[wl] : 0;
}

// the row of table t - 1 that row q of table t came from, -1: none (a link at
// or past N_{t-1} cannot come from an exported row and counts as none)
__host__ __device__ inline int32_t traj_link(const TrajWin &w, uint32_t t, uint32_t q, uint32_t n_prev)
{
    const int32_t p = w.link[traj_at(w, t, q)];
    return (p >= 0 && (uint32_t)p < n_prev) ? p : -1;
}

// end[t][q] once next[t] is final (n tables)
__host__ __device__ inline int32_t traj_end(const TrajWin &w, uint32_t n, uint32_t t, uint32_t q)
{
    if (t + 1 >= n) return kTrajEndWindow;
    if (w.next[traj_at(w, t, q)] >= 0) return kTrajEndNone;
    const uint32_t wl = (uint32_t)w.world[traj_at(w, t, q)] - w.world_offset;
    return (wl < w.Wx && w.mark[(size_t)traj_slot(w, t + 1) * w.Wx + wl]) ? kTrajEndReset : kTrajEndDied;
}

struct TrajParams {
    float gamma, gl, death_reward;   // gl = gamma * lambda, rounded once
};

// The sweep's element (t, q), q < N_t: writes end[t][q]; a row of the last
// table gets adv = 0, ret = value; a lifeline end -- a row of table <= n - 2
// with end != 0, or any row of table n - 2 -- computes its own adv / ret and
// walks `link` backwards, writing every earlier (t', q') of its lifeline.  Each
// (t, q) is written by exactly one element: a row with a successor belongs to
// the lifeline of that successor's end.
__host__ __device__ inline void traj_sweep(const TrajWin &w, const TrajParams &P, uint32_t n, uint32_t t, uint32_t q)
{
    const size_t i = traj_at(w, t, q);
    const int32_t e = traj_end(w, n, t, q);
    w.end[i] = e;
    if (e == kTrajEndWindow) {
        w.adv[i] = 0.0f;
        w.ret[i] = w.value[i];
        return;
    }
    if (e == kTrajEndNone && t + 2 != n) return;   // its successor's lifeline end writes it
    float adv;
    if (e == kTrajEndNone) {
        const size_t j = traj_at(w, t + 1, (uint32_t)w.next[i]);
        adv = traj_add(traj_add(w.reward[j], traj_mul(P.gamma, w.value[j])), -w.value[i]);
    } else if (e == kTrajEndDied) {
        adv = traj_add(P.death_reward, -w.value[i]);
    } else {
        adv = 0.0f;
    }
    w.adv[i] = adv;
    w.ret[i] = traj_add(adv, w.value[i]);
    size_t cur = i;
    while (t > 0) {
        const int32_t p = traj_link(w, t, q, w.count[traj_slot(w, t - 1)]);
        if (p < 0) break;
        const size_t k = traj_at(w, t - 1, (uint32_t)p);
        const float delta = traj_add(traj_add(w.reward[cur], traj_mul(P.gamma, w.value[cur])), -w.value[k]);
        adv = traj_add(delta, traj_mul(P.gl, adv));
        w.adv[k] = adv;
        w.ret[k] = traj_add(adv, w.value[k]);
        cur = k;
        q = (uint32_t)p;
        --t;
    }
}

}  // namespace mbots
