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
    // the opt-in parts (mbots_traj_open_ex; each null while its flag is off)
    int32_t *seq_id, *seq_pos;              // [horizon][max_rows]: the row's sequence and its position in it
    uint32_t *blk;                          // [horizon][ceil(max_rows / 256)] starts per 256-row block, then
                                            // their exclusive scan; one more word: the total S
    uint8_t *rec;                           // [horizon][max_rows][rec_bytes] rollout records
    float *hidden;                          // [horizon][max_rows][16] HiddenState
    uint8_t *amask;                         // [horizon][max_rows] bit i: Action[r][i] != 0
    uint32_t rec_bytes;                     // 64, or 96 with the real depth
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

// ---- sequences (mbots_traj_sequences) and batches (mbots_traj_batch) ----
constexpr uint32_t kTrajBlock = 256;   // rows per block of the start count
constexpr uint32_t kTrajHidden = 16;

// push, state part: the mask of row r's Action, and granule g (four floats; a
// row holds four) of the table's HiddenState rows [0, lim), which are one
// contiguous copy into the slot
__host__ __device__ inline void traj_push_mask(const TrajWin &w, uint32_t s, uint32_t r, const int32_t *action)
{
    uint32_t m = 0;
    for (uint32_t k = 0; k < 6u; ++k) m |= (action[(size_t)6 * r + k] != 0 ? 1u : 0u) << k;
    w.amask[(size_t)s * w.max_rows + r] = (uint8_t)m;
}
__host__ __device__ inline void traj_push_hidden(const TrajWin &w, uint32_t s, size_t g, const float *hidden)
{
    float *dst = w.hidden + ((size_t)s * w.max_rows * kTrajHidden + 4u * g);
    const float *src = hidden + 4u * g;
#ifdef __HIP_DEVICE_COMPILE__
    // (both 16-byte aligned: the column's allocation, and slots of whole rows)
    *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
#else
    for (int k = 0; k < 4; ++k) dst[k] = src[k];
#endif
}

// row q < N_t of table t starts a sequence: the window's first table, or no
// predecessor among the rows of table t - 1
__host__ __device__ inline bool traj_is_start(const TrajWin &w, uint32_t t, uint32_t q)
{
    return t == 0u || traj_link(w, t, q, w.count[traj_slot(w, t - 1u)]) < 0;
}

// the start (t, q) of sequence `id` walks `next` forward to the first row with
// end != 0 (at most n - t rows: the last table's rows all end), writing the id
// and the position into every row it passes -- the sweep's walk, forwards
__host__ __device__ inline void traj_seq_walk(const TrajWin &w, uint32_t n, uint32_t t, uint32_t q, uint32_t id)
{
    for (uint32_t k = 0; t < n; ++k, ++t) {
        const size_t i = traj_at(w, t, q);
        w.seq_id[i] = (int32_t)id;
        w.seq_pos[i] = (int32_t)k;
        if (w.end[i] != kTrajEndNone) break;
        q = (uint32_t)w.next[i];
    }
}

// the outputs of a batch of sequences [lo, lo + B): include/mbots.h
// mbots_traj_batch (any pointer may be null), with the index the obs and gather
// kernels read (rows / t0: the caller's arrays or the window's scratch)
struct TrajBatch {
    int32_t *rows, *t0, *len, *end;
    float *reward, *value, *adv, *ret;
    uint8_t *action_in;
    float *hidden0;
};

// the scatter's element (t, q): a row of a sequence of the batch writes its own
// entries (the arrays were filled with the padding before)
__host__ __device__ inline void traj_batch_row(const TrajWin &w, const TrajBatch &o, uint32_t lo, uint64_t B,
                                               uint32_t t, uint32_t q)
{
    const size_t i = traj_at(w, t, q);
    const uint32_t id = (uint32_t)w.seq_id[i] - lo;   // (below lo: wraps past B)
    if (id >= B) return;
    const uint32_t k = (uint32_t)w.seq_pos[i];
    const size_t j = (size_t)k * B + id;
    if (o.rows) o.rows[j] = (int32_t)q;
    if (o.reward) o.reward[j] = w.reward[i];
    if (o.value) o.value[j] = w.value[i];
    if (o.adv) o.adv[j] = w.adv[i];
    if (o.ret) o.ret[j] = w.ret[i];
    if (o.action_in) o.action_in[j] = w.amask[i];
    if (k == 0u) {
        if (o.t0) o.t0[id] = (int32_t)t;
        if (o.hidden0)
            for (uint32_t c = 0; c < kTrajHidden; ++c)
                o.hidden0[(size_t)id * kTrajHidden + c] = w.hidden[i * kTrajHidden + c];
    }
    const int32_t e = w.end[i];
    if (e != kTrajEndNone) {
        if (o.len) o.len[id] = (int32_t)k + 1;
        if (o.end) o.end[id] = e;
    }
}

// the stored record of output row (k, b) of a batch: null for padding
__host__ __device__ inline const uint8_t *traj_batch_record(const TrajWin &w, const int32_t *rows, const int32_t *t0,
                                                            uint64_t B, uint64_t o)
{
    const int32_t q = rows[o];
    if (q < 0) return nullptr;
    const uint32_t t = (uint32_t)t0[o % B] + (uint32_t)(o / B);
    return w.rec + traj_at(w, t, (uint32_t)q) * w.rec_bytes;
}

// construct_obs's float c < 69 of a rollout record (unpack_rollout_kernel's
// val(); depth: the record holds the depth bytes at 64)
__host__ __device__ inline uint32_t traj_obs_bits(const uint8_t *q, bool depth, uint32_t c)
{
    float f;
    if (c < 32u) f = (float)q[depth ? 64u + c : c];
    else if (c < 35u) return reinterpret_cast<const uint32_t *>(q)[8u + (c - 32u)];
    else if (c < 67u) f = (float)(int8_t)q[c - 35u];
    else return reinterpret_cast<const uint32_t *>(q)[11u + (c - 67u)];
    union { float f; uint32_t u; } b;
    b.f = f;
    return b.u;
}

}  // namespace mbots
