// mbots_policy.hip -- the device actor's kernels (mbots_policy.hpp; DESIGN.md
// "Device actor"): per-species policy nets on v_mfma_f32_16x16x4_f32, action
// sampling from the counter RNG and the Action / HiddenState write, one
// persistent launch over 64-row tiles of the current table; and the learner's
// half (DESIGN.md "Differentiable evaluate"): the same nets on recorded rows,
// and their parameter gradients from a persistent backward kernel.
#include "mbots_kernels.hpp"
#include "mbots_policy.hpp"

#include <algorithm>

namespace mbots {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPolRows = 64;        // rows per tile (a block of 4 waves)
constexpr int kPolStride = 132;     // floats per LDS row: 128 + 4, so the 16 rows x 4 k of an A
                                    // fragment and the 16 x 4 results of a C tile each hit 64 banks
constexpr int kPolLogitStride = 8, kPolMemStride = 16;
// two activation tiles, the heads' outputs, and three words per row for the row's world
constexpr size_t kPolLds =
    (2 * kPolRows * kPolStride + kPolRows * (kPolLogitStride + 1 + kPolMemStride + 3)) * sizeof(float);

// One Linear over the tile's 64 rows: out[r][j] = act(bias[j] + sum_k x[r][k] W[j][k]),
// k ascending.  Wave (wv - woff) & 3 takes column tiles jt = that, that + 4 for
// all four 16-row tiles: up to 8 independent accumulators per k-step, the
// layer's weights read once per block, straight from L2 in fragment order (64
// contiguous floats per (k-step, column tile)).  The C operand starts as the
// broadcast bias; columns >= L.out (the heads' pads) are never stored.
//
// kBack (the backward pass's input gradients, L the transposed layer with a +0
// bias): the epilogue stores (add[r][j] +) acc times the derivative of
// activation `act` at the value dst[r][j] holds -- the forward's output, which
// the gradient replaces in place; act < 0: no derivative factor.  kSrc: floats
// per row of `src`.  kSigmoid: the gate head -- the activation is pol_sigmoid,
// whatever `act` says.
template <bool kBack = false, int kSrc = kPolStride, bool kSigmoid = false>
__device__ __forceinline__ void pol_layer(const PolLayer &L, int act, const float *src, float *dst,
                                          uint32_t dst_stride, uint32_t wv, uint32_t woff, uint32_t lane,
                                          const float *add = nullptr)
{
    const uint32_t nt = L.nt, nks = L.kp >> 2;
    const uint32_t j0 = (wv - woff) & 3u, j1 = j0 + 4u;
    if (j0 >= nt) return;
    const bool two = j1 < nt;
    const uint32_t c = lane & 15u, q = lane >> 4;
    f32x4 acc0[4], acc1[4];
    {
        const float b0 = L.b[j0 * 16u + c], b1 = two ? L.b[j1 * 16u + c] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            acc0[mt] = f32x4{b0, b0, b0, b0};
            acc1[mt] = f32x4{b1, b1, b1, b1};
        }
    }
    const float *wp0 = L.w + (size_t)j0 * 64u + lane, *wp1 = L.w + (size_t)j1 * 64u + lane;
    const size_t wstep = (size_t)nt * 64u;
    const float *xa = src + c * kSrc + q;
    // (a guarded register ring loading the B fragments four k-steps ahead
    // measured slower, 5.9 against 5.0 ms at 65536 worlds; the branch-free pair
    // below 4.85 against 4.90 for one k-step per pass)
    if (two) {
        // two k-steps per pass (nks is even), the next pass's B fragments loaded
        // before this pass's MFMAs (the last pass reloads its own: no branch)
        float n00 = wp0[0], n01 = wp0[wstep], n10 = wp1[0], n11 = wp1[wstep];
        for (uint32_t ks = 0; ks < nks; ks += 2u) {
            const float b00 = n00, b01 = n01, b10 = n10, b11 = n11;
            const size_t kn = (size_t)min(ks + 2u, nks - 2u) * wstep;
            n00 = wp0[kn];
            n01 = wp0[kn + wstep];
            n10 = wp1[kn];
            n11 = wp1[kn + wstep];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float a = xa[mt * 16 * kSrc + 4u * ks];
                acc0[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b00, acc0[mt], 0, 0, 0);
                acc1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b10, acc1[mt], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float a = xa[mt * 16 * kSrc + 4u * ks + 4u];
                acc0[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b01, acc0[mt], 0, 0, 0);
                acc1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b11, acc1[mt], 0, 0, 0);
            }
        }
    } else {
        for (uint32_t ks = 0; ks < nks; ++ks) {
            const float b0 = wp0[ks * wstep];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float a = xa[mt * 16 * kSrc + 4u * ks];
                acc0[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0[mt], 0, 0, 0);
            }
        }
    }
    // C / D: column lane & 15, row (lane >> 4) * 4 + register
    const uint32_t col0 = j0 * 16u + c, col1 = j1 * 16u + c;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = (uint32_t)mt * 16u + q * 4u + (uint32_t)r;
            if constexpr (kBack) {
                if (col0 < L.out) {
                    float *o = dst + row * dst_stride + col0;
                    float v = acc0[mt][r];
                    if (add) v = add[row * dst_stride + col0] + v;
                    if (act >= 0) v = v * pol_activation_grad(act, *o);
                    *o = v;
                }
                if (two && col1 < L.out) {
                    float *o = dst + row * dst_stride + col1;
                    float v = acc1[mt][r];
                    if (add) v = add[row * dst_stride + col1] + v;
                    if (act >= 0) v = v * pol_activation_grad(act, *o);
                    *o = v;
                }
            } else {
                if constexpr (kSigmoid) {
                    if (col0 < L.out) dst[row * dst_stride + col0] = pol_sigmoid(acc0[mt][r]);
                    if (two && col1 < L.out) dst[row * dst_stride + col1] = pol_sigmoid(acc1[mt][r]);
                } else {
                    if (col0 < L.out) dst[row * dst_stride + col0] = pol_activation(act, acc0[mt][r]);
                    if (two && col1 < L.out) dst[row * dst_stride + col1] = pol_activation(act, acc1[mt][r]);
                }
            }
        }
}

struct PolActArgs {
    const uint32_t *totals;
    const int32_t *scount, *row_base;
    const uint8_t *depth;
    const int8_t *sem;
    const int32_t *health;
    const float *pos, *sur;
    const float *hidden_in;     // the HiddenState column as its readers see it
    int32_t *action;            // null: MBOTS_ACT_NO_WRITE
    float *hidden_out;
    int32_t *action_out;        // [out_rows] each, any may be null
    float *logp_out, *value_out;
    const uint32_t *draw;
    uint32_t out_rows, W, Wx, world_offset, seed, greedy;
};

// A net's scalars and layers as the tile body reads them.  The four nets of a
// one-group launch are kernel arguments and read where they lie (scalar
// loads); an entry of the groups' table lies in device memory, whose loads the
// compiler cannot prove uniform, so each value goes through an SGPR.
template <bool kTable> __device__ __forceinline__ uint32_t pol_u(uint32_t v)
{
    if constexpr (kTable) return uniform(v);
    else return v;
}
// The lane index behind a barrier the optimiser cannot look through: what a
// gated net's extra layers derive from it (their per-lane addresses) is worked
// out where they run, not hoisted out of the surrounding loop and kept in
// registers across the ungated path.
__device__ __forceinline__ uint32_t pol_opaque(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float *pol_uniform_ptr(float *p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint64_t lo = uniform((uint32_t)v), hi = uniform((uint32_t)(v >> 32));
    return reinterpret_cast<float *>((hi << 32) | lo);
}
template <bool kTable> __device__ __forceinline__ decltype(auto) pol_pick(const PolLayer &l)
{
    if constexpr (kTable) {
        PolLayer u;
        u.w = pol_uniform_ptr(l.w);
        u.b = pol_uniform_ptr(l.b);
        u.in = uniform(l.in);
        u.out = uniform(l.out);
        u.kp = uniform(l.kp);
        u.nt = uniform(l.nt);
        u.act = uniform(l.act);
        return u;
    } else {
        return (l);   // the kernel argument itself, by reference
    }
}

// One tile of policy_act: rows [r0, r0 + nr) of species sp + 1 (one (group,
// species) segment, `ghost`: the shard ghost's) through `net`, sampled and
// written.  kTable: `net` is an entry of the groups' table.  kGate: a net of the
// launch may be gated (without, the gate's code is not in the kernel at all: a
// manager none of whose nets has a gate launches the kernels it always did).
template <bool kTable, bool kGate>
__device__ __forceinline__ void pol_act_tile(const PolActArgs &A, const PolNet &net, bool ghost, uint32_t sp,
                                             uint32_t r0, uint32_t nr, uint32_t draw, float *s_pol)
{
    float *buf0 = s_pol, *buf1 = s_pol + kPolRows * kPolStride;
    float *s_logit = buf1 + kPolRows * kPolStride;
    float *s_val = s_logit + kPolRows * kPolLogitStride;
    float *s_mem = s_val + kPolRows;
    uint32_t *s_win = reinterpret_cast<uint32_t *>(s_mem + kPolRows * kPolMemStride);
    uint32_t *s_w = s_win + kPolRows, *s_k = s_w + kPolRows;
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const bool mem_in = (pol_u<kTable>(net.flags) & kPolMemoryIn) != 0u;
    const uint32_t n_trunk = pol_u<kTable>(net.n_trunk);
    const bool has_memory = pol_u<kTable>(net.has_memory) != 0u;
    const bool gated = kGate && pol_u<kTable>(net.gated) != 0u;

    // ---- stage the tile's inputs, coalesced, as the f32 tile X[64][Kp] ----
    {
        const uint32_t row = (t & 127u) >> 1, half = t & 1u;
        float *x = buf0 + row * kPolStride + (t < 128u ? 0u : 35u) + half * 16u;
        if (row < nr) {
            const uint4 g = t < 128u ? reinterpret_cast<const uint4 *>(A.depth + (size_t)r0 * kSensor)[t]
                                     : reinterpret_cast<const uint4 *>(A.sem + (size_t)r0 * kSensor)[t - 128u];
            const uint32_t wds[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t b = (wds[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                x[i] = t < 128u ? (float)b : (float)(int8_t)b;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = 0.0f;
        }
    }
    if (t < (uint32_t)kPolRows) {
        float *x = buf0 + t * kPolStride;
        int32_t hp = 0;
        float2 ps = make_float2(0.0f, 0.0f), su = ps;
        if (t < nr) {
            hp = A.health[r0 + t];
            ps = reinterpret_cast<const float2 *>(A.pos)[r0 + t];
            su = reinterpret_cast<const float2 *>(A.sur)[r0 + t];
        }
        x[32] = __int_as_float(hp);
        x[33] = ps.x;
        x[34] = ps.y;
        x[67] = su.x;
        x[68] = su.y;
        if (!mem_in) x[69] = x[70] = x[71] = 0.0f;
        else x[85] = x[86] = x[87] = 0.0f;
    }
    if (mem_in) {
        const uint32_t row = t >> 2, g = t & 3u;
        float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row < nr) h = reinterpret_cast<const float4 *>(A.hidden_in + (size_t)r0 * kHidden)[t];
        float *x = buf0 + row * kPolStride + kPolObs + 4u * g;
        x[0] = h.x;
        x[1] = h.y;
        x[2] = h.z;
        x[3] = h.w;
    }
    // ---- wave 3: each row's world and its index k inside the (world, species)
    // segment, for the epilogue's RNG key.  The first row's world by a 64-ary
    // search of row_base (three rounds at 65536 worlds), then the next 64
    // worlds' bases as a window in LDS that the rows bisect ----
    if (wv == 3u) {
        const uint32_t r = r0 + lane;
        uint32_t w = A.Wx, k = 0;
        if (ghost) {
            k = r - (uint32_t)A.row_base[4u * A.Wx + sp];
        } else {
            uint32_t lo = 0, n = A.Wx;   // the world lies in [lo, lo + n), row_base[lo] <= r0
            while (n > 1u) {
                const uint32_t step = (n + 63u) >> 6, end = lo + n, p = lo + (lane + 1u) * step;
                const bool ok = p < end && (uint32_t)A.row_base[4u * p + sp] <= r0;
                lo += (uint32_t)__popcll(ballot64(ok)) * step;
                n = min(step, end - lo);
            }
            const uint32_t w0 = lo, pw = w0 + 1u + lane;
            s_win[lane] = pw < A.Wx ? (uint32_t)A.row_base[4u * pw + sp] : 0xFFFFFFFFu;
            wave_sync();
            if (lane < nr) {
                uint32_t c = 0;   // window entries <= r: the row's world is w0 + c
                for (uint32_t s = 32u; s; s >>= 1)
                    if (s_win[c + s - 1u] <= r) c += s;
                if (c == 63u && s_win[63] <= r) c = 64u;
                w = w0 + c;
                if (c == 64u) {   // past the window (a long run of worlds without the species)
                    uint32_t hi = A.Wx;
                    while (hi - w > 1u) {
                        const uint32_t mid = (w + hi) >> 1;
                        if ((uint32_t)A.row_base[4u * mid + sp] <= r) w = mid;
                        else hi = mid;
                    }
                }
                k = r - (uint32_t)A.row_base[4u * w + sp];
            }
        }
        s_w[lane] = w;
        s_k[lane] = k;
    }
    __syncthreads();

    // ---- trunk: ping-pong between the two tiles ----
    float *cur = buf0, *oth = buf1;
    for (uint32_t l = 0; l < n_trunk; ++l) {
        pol_layer(pol_pick<kTable>(net.trunk[l]), (int)pol_u<kTable>(net.trunk[l].act), cur, oth, kPolStride, wv, 0u,
                  lane);
        __syncthreads();
        float *sw = cur;
        cur = oth;
        oth = sw;
    }
    // ---- heads, all reading the trunk's last tile `cur` ----
    pol_layer(pol_pick<kTable>(net.actor[0]), kActRelu, cur, oth, kPolStride, wv, 0u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.actor[1]), kActIdentity, oth, s_logit, kPolLogitStride, wv, 0u, lane);
    if (has_memory) pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_mem, kPolMemStride, wv, 1u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.critic[0]), kActRelu, cur, oth, kPolStride, wv, 0u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.critic[1]), kActIdentity, oth, s_val, 1u, wv, 0u, lane);
    __syncthreads();
    // the gate head's z, in the tile the critic has done with (DESIGN.md "Gated memory head")
    float *s_z = oth;
    if (gated) {
        pol_layer<false, kPolStride, true>(pol_pick<kTable>(net.gate), kActSigmoid, cur, s_z, kPolMemStride, wv, 0u,
                                           pol_opaque(lane));
        __syncthreads();
    }

    // ---- epilogue: sample, log-probability, the table's writes ----
    if (t < nr) {
        const uint32_t r = r0 + t;
        const uint32_t w = s_w[t], k = s_k[t];
        float z[kPolActions];
#pragma unroll
        for (int i = 0; i < kPolActions; ++i) z[i] = s_logit[t * kPolLogitStride + i];
        const float u = pol_uniform(A.seed, draw, A.world_offset + w, sp + 1u, k);
        float logp;
        const int32_t a = pol_sample(z, u, A.greedy != 0u, &logp);
        if (A.action) {
            int2 *o = reinterpret_cast<int2 *>(A.action + (size_t)r * 6u);
            o[0] = make_int2(a == 0, a == 1);
            o[1] = make_int2(a == 2, a == 3);
            o[2] = make_int2(a == 4, a == 5);
        }
        if (r < A.out_rows) {
            if (A.action_out) A.action_out[r] = a;
            if (A.logp_out) A.logp_out[r] = logp;
            if (A.value_out) A.value_out[r] = s_val[t];
        }
    }
    if (has_memory && A.hidden_out) {
        const uint32_t row = t >> 2, g = t & 3u;
        if (row < nr) {
            const float *m = s_mem + row * kPolMemStride + 4u * g;
            float4 o = make_float4(m[0], m[1], m[2], m[3]);
            if (gated) {   // (hidden_out may be the column hidden_in is: this thread reads before it writes)
                const float4 h = reinterpret_cast<const float4 *>(A.hidden_in + (size_t)r0 * kHidden)[t];
                const float *z = s_z + row * kPolMemStride + 4u * g;
                o = make_float4(pol_gate_blend(z[0], o.x, h.x), pol_gate_blend(z[1], o.y, h.y),
                                pol_gate_blend(z[2], o.z, h.z), pol_gate_blend(z[3], o.w, h.w));
            }
            reinterpret_cast<float4 *>(A.hidden_out + (size_t)r0 * kHidden)[t] = o;
        }
    }
    __syncthreads();
}

template <bool kGate> __global__ __launch_bounds__(256, 2) void policy_act_kernel(PolActArgs A, PolNets P)
{
    extern __shared__ float s_pol[];

    // the table's eight species segments: the exported rows of species 1..4,
    // then the shard ghost's (after row N); a tile never straddles two
    uint32_t seg_len[8], seg_start[8];
    {
        uint32_t run = 0;
        for (int s = 0; s < 4; ++s) {
            seg_len[s] = uniform(A.totals[1 + s]);
            seg_start[s] = run;
            run += seg_len[s];
        }
        run = uniform(A.totals[0]);
        for (int s = 0; s < 4; ++s) {
            seg_len[4 + s] = A.W > A.Wx ? uniform((uint32_t)A.scount[4u * A.Wx + s]) : 0u;
            seg_start[4 + s] = run;
            run += seg_len[4 + s];
        }
    }
    const uint32_t draw = uniform(*A.draw);

    for (uint32_t tile = blockIdx.x;; tile += gridDim.x) {
        uint32_t seg = 0, rest = tile;
        for (; seg < 8u; ++seg) {
            const uint32_t nt = (seg_len[seg] + kPolRows - 1u) / kPolRows;
            if (rest < nt) break;
            rest -= nt;
        }
        if (seg >= 8u) break;
        const uint32_t sp = seg & 3u;   // species - 1
        const uint32_t r0 = seg_start[seg] + rest * kPolRows;
        const uint32_t nr = min((uint32_t)kPolRows, seg_len[seg] - rest * kPolRows);
        pol_act_tile<false, kGate>(A, P.net[sp], seg >= 4u, sp, r0, nr, draw, s_pol);
    }
}

// ---- policy groups (mbots_policy.hpp; DESIGN.md "Policy groups") ----
// The segments of a grouped table in row order: entry s * G + g the exported
// rows of (group g, species s + 1), then the shard ghost's four.  Each block
// builds the table in its prologue -- first row, length, and the inclusive scan
// of the tile counts, which every tile then bisects -- behind the tile's LDS.
// (A copy of the tile's net descriptor in LDS, so that a layer starts from LDS
// and not from a load of the table, measured no faster: 6.14 against 6.09 ms
// with 32 groups at 65536 worlds.)
constexpr uint32_t kPolMaxSegs = 4u * kPolMaxGroups + 4u;
constexpr size_t kPolGroupLds = kPolLds + (3u * kPolMaxSegs + 4u) * sizeof(uint32_t);
static_assert(kPolGroupLds <= 80u * 1024u, "two blocks of policy_act_groups_kernel share a compute unit's LDS");
static_assert(kPolMaxSegs <= 2u * 256u, "two segment entries per thread");

template <bool kGate> __global__ __launch_bounds__(256, 2) void policy_act_groups_kernel(PolActArgs A, PolGroups G)
{
    extern __shared__ float s_pol[];
    uint32_t *s_start = reinterpret_cast<uint32_t *>(s_pol) + kPolLds / sizeof(uint32_t);
    uint32_t *s_len = s_start + kPolMaxSegs, *s_scan = s_len + kPolMaxSegs, *s_wsum = s_scan + kPolMaxSegs;
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint32_t nG = G.G, nseg = 4u * nG + 4u;
    {
        uint32_t sp_end[4], run = 0;
        for (int s = 0; s < 4; ++s) {
            run += uniform(A.totals[1 + s]);
            sp_end[s] = run;
        }
        uint32_t c[2];
        for (uint32_t i = 0; i < 2u; ++i) {
            const uint32_t e = 2u * t + i;
            uint32_t start = 0, len = 0;
            if (e < 4u * nG) {
                const uint32_t s = e / nG, g = e - s * nG;
                const uint32_t end = s == 0u ? sp_end[0] : s == 1u ? sp_end[1] : s == 2u ? sp_end[2] : sp_end[3];
                start = pol_group_edge(A.row_base, A.Wx, G.first[g], s, end);
                len = pol_group_edge(A.row_base, A.Wx, G.first[g + 1u], s, end) - start;
            } else if (e < nseg && A.W > A.Wx) {
                const uint32_t s = e - 4u * nG;
                start = A.totals[0];
                for (uint32_t q = 0; q < s; ++q) start += (uint32_t)A.scount[4u * A.Wx + q];
                len = (uint32_t)A.scount[4u * A.Wx + s];
            }
            if (e < kPolMaxSegs) {
                s_start[e] = start;
                s_len[e] = len;
            }
            c[i] = (len + kPolRows - 1u) / kPolRows;
        }
        // the block-wide inclusive scan of the tile counts: pairs, waves, the four wave sums
        uint32_t incl = c[0] + c[1];
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) s_wsum[wv] = incl;
        __syncthreads();
        for (uint32_t q = 0; q < wv; ++q) incl += s_wsum[q];
        if (2u * t < kPolMaxSegs) s_scan[2u * t] = incl - c[1];
        if (2u * t + 1u < kPolMaxSegs) s_scan[2u * t + 1u] = incl;
        __syncthreads();
    }
    const uint32_t tiles = uniform(s_scan[nseg - 1u]);
    const uint32_t draw = uniform(*A.draw);

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // the first entry whose scan exceeds the tile (entries without rows are passed over)
        uint32_t lo = 0, hi = nseg - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_scan[mid] > tile) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t e = uniform(lo);
        const uint32_t rest = tile - (e ? uniform(s_scan[e - 1u]) : 0u);
        const bool ghost = e >= 4u * nG;
        const uint32_t sp = ghost ? e - 4u * nG : e / nG;   // species - 1
        const uint32_t g = ghost ? G.ghost : e - sp * nG;
        const uint32_t len = uniform(s_len[e]);
        const uint32_t r0 = uniform(s_start[e]) + rest * kPolRows;
        const uint32_t nr = min((uint32_t)kPolRows, len - rest * kPolRows);
        pol_act_tile<true, kGate>(A, G.table[4u * g + sp], ghost, sp, r0, nr, draw, s_pol);
    }
}

// [lo, hi) of every (group, species) among the exported rows of the current table
static_assert(4u * kPolMaxGroups <= 256u, "policy_segments_kernel: one thread per (group, species) in its one block");
__global__ __launch_bounds__(256) void policy_segments_kernel(const uint32_t *totals, const int32_t *row_base,
                                                              uint32_t Wx, PolGroups G, int32_t *out)
{
    const uint32_t e = threadIdx.x;
    if (e >= 4u * G.G) return;
    const uint32_t g = e >> 2, s = e & 3u;
    uint32_t end = 0;
    for (uint32_t q = 0; q <= s; ++q) end += totals[1u + q];
    out[2u * e] = (int32_t)pol_group_edge(row_base, Wx, G.first[g], s, end);
    out[2u * e + 1u] = (int32_t)pol_group_edge(row_base, Wx, G.first[g + 1u], s, end);
}

__global__ void policy_draw_next_kernel(uint32_t *draw) { *draw += 1u; }

// one layer's weights into the fragment order / the padded bias, over the blocks of a grid row
__device__ __forceinline__ void pol_repack_layer(const PolUpload &L)
{
    const uint32_t nw = L.kp * L.nt * 16u, nb = L.nt * 16u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nw + nb; i += gridDim.x * 256u) {
        if (i < nw) {
            const uint32_t l = i & 63u, f = i >> 6, jt = f % L.nt, ks = f / L.nt;
            const uint32_t j = jt * 16u + (l & 15u), k = 4u * ks + (l >> 4);
            const uint32_t ld = L.ld ? L.ld : L.out;
            L.w_dst[i] = (j < L.out && k < L.in)
                             ? (L.tr ? L.w_src[(size_t)k * ld + L.off + j] : L.w_src[(size_t)j * L.in + k])
                             : 0.0f;
        } else {
            const uint32_t j = i - nw;
            L.b_dst[j] = (j < L.out && L.b_src) ? L.b_src[j] : 0.0f;
        }
    }
}

// one block column per layer
__global__ __launch_bounds__(256) void policy_repack_kernel(PolUploads U) { pol_repack_layer(U.l[blockIdx.y]); }

__global__ __launch_bounds__(256) void policy_activation_kernel(int act, const float *x, float *y, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        y[i] = pol_activation_any(act, x[i]);
}

// ---- evaluate and its backward pass (mbots_policy.hpp; DESIGN.md "Differentiable
// evaluate") ----
constexpr int kPolTile = kPolRows * kPolStride;   // floats of one LDS tile
constexpr int kPolStashTiles = kPolMaxTrunk - 1;  // outputs of all trunk layers but the last, per block
constexpr size_t kPolEvalLds = (2 * kPolTile + kPolRows * (kPolLogitStride + 1)) * sizeof(float);
constexpr size_t kPolGradLds = (4 * kPolTile + kPolRows * (kPolLogitStride + 1)) * sizeof(float);

// the tile's inputs from the dense rows: X[64][kp], +0 for the pads and the rows past nr
__device__ __forceinline__ void pol_stage_dense(float *x, const PolEvalIO &A, uint64_t r0, uint32_t nr, uint32_t kp,
                                                bool mem_in, uint32_t t)
{
    for (uint32_t i = t; i < (uint32_t)kPolRows * kp; i += 256u) {
        const uint32_t row = i / kp, k = i - row * kp;
        float v = 0.0f;
        if (row < nr) {
            if (k < (uint32_t)kPolObs) v = A.obs[(r0 + row) * kPolObs + k];
            else if (mem_in && k < (uint32_t)(kPolObs + kHidden)) v = A.hidden[(r0 + row) * kHidden + (k - kPolObs)];
        }
        x[row * kPolStride + k] = v;
    }
}

__device__ __forceinline__ void pol_copy_tile(float *dst, const float *src, uint32_t t)
{
    for (uint32_t i = t; i < (uint32_t)kPolTile / 4u; i += 256u)
        reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
}

// One layer's parameter gradients over the tile: dW[j][k] continues its chain
// fmaf(d[r][j], x[r][k], dW[j][k]) over the 64 rows in ascending order -- the
// k-steps of the matrix instruction, A the transposed d, B the layer's input x
// -- and db[j] its chain of adds.  The chains live in the block's slab (dW as
// the C fragments of its 16 x 16 tiles) and start at +0 on the block's first
// tile.  Wave w takes the out-feature tiles w and w + 4, four in-feature tiles
// at a time; columns of x past kp and what they produce are never read back.
// kD: floats per row of `d`.
template <int kD = kPolStride>
__device__ __forceinline__ void pol_grad_w(const PolLayer &L, const float *d, const float *x, float *sw, float *sb,
                                           bool first, uint32_t wv, uint32_t lane, uint32_t t)
{
    const uint32_t nt = L.nt, nkt = pol_grad_nkt(L.kp);
    const uint32_t c = lane & 15u, q = lane >> 4;
    for (uint32_t jt = wv; jt < nt; jt += 4u) {
        const float *da = d + q * kD + jt * 16u + c;
        for (uint32_t kt0 = 0; kt0 < nkt; kt0 += 4u) {
            const uint32_t nk = min(4u, nkt - kt0);
            f32x4 acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (!first && (uint32_t)u < nk) {
                    const float *p = sw + ((size_t)(jt * nkt + kt0 + u) * 4u) * 64u + lane;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[u][r] = p[r * 64];
                }
            }
            const float *xb = x + q * kPolStride + kt0 * 16u + c;
            if (nk == 4u) {
                for (uint32_t s = 0; s < (uint32_t)kPolRows / 4u; ++s) {
                    const float a = da[s * 4u * kD];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[s * 4u * kPolStride + u * 16], acc[u], 0, 0, 0);
                }
            } else {
                for (uint32_t s = 0; s < (uint32_t)kPolRows / 4u; ++s) {
                    const float a = da[s * 4u * kD];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if ((uint32_t)u < nk)
                            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[s * 4u * kPolStride + u * 16], acc[u], 0,
                                                                          0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((uint32_t)u < nk) {
                    float *p = sw + ((size_t)(jt * nkt + kt0 + u) * 4u) * 64u + lane;
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[r * 64] = acc[u][r];
                }
        }
    }
    if (t < nt * 16u) {
        float acc = first ? 0.0f : sb[t];
        for (int r = 0; r < kPolRows; ++r) acc = acc + d[r * kD + t];
        sb[t] = acc;
    }
}

struct PolGradDev {
    PolNet back;          // the transposed layers (trunk 1.., heads), each with a +0 bias
    PolGradSlabs slabs;
    float *stash;         // [blocks][kPolStashTiles][kPolTile]
};

// One tile of evaluate: rows [r0, r0 + nr) through `net`.  kGrad false: their
// logp, value and entropy.  kGrad true: the forward again (outputs of the inner
// trunk layers to the block's stash), d loss / d logits, then layer by layer
// from the heads down the parameter gradients into the block's slab (layer
// l's dW at sw[l], db at sb[l]; `first`: the chains start here) and the input
// gradients in place of the layer outputs.  kTable: `net`, `back`, sw and sb
// lie in device memory (the grouped calls' descriptor table).  t, wv, lane: the
// thread, its wave (uniform) and its lane, which the kernel works out once.
template <bool kGrad, bool kTable>
__device__ __forceinline__ void pol_eval_tile(const PolEvalIO &A, const PolNet &net, const PolNet &back,
                                              const uint32_t *sw, const uint32_t *sb, float *slab, float *stash,
                                              uint64_t r0, uint32_t nr, bool first, float *s_pol, uint32_t t, uint32_t wv,
                                              uint32_t lane)
{
    float *buf0 = s_pol, *buf1 = s_pol + kPolTile;
    float *tail = s_pol + (kGrad ? 4 : 2) * kPolTile;
    float *s_logit = tail, *s_val = tail + kPolRows * kPolLogitStride;
    const bool mem_in = (pol_u<kTable>(net.flags) & kPolMemoryIn) != 0u;

    pol_stage_dense(buf0, A, r0, nr, pol_u<kTable>(net.trunk[0].kp), mem_in, t);
    __syncthreads();
    float *cur = buf0, *oth = buf1;
    for (uint32_t l = 0; l < pol_u<kTable>(net.n_trunk); ++l) {
        pol_layer(pol_pick<kTable>(net.trunk[l]), (int)pol_u<kTable>(net.trunk[l].act), cur, oth, kPolStride, wv, 0u,
                  lane);
        __syncthreads();
        float *sw_ = cur;
        cur = oth;
        oth = sw_;
        if (kGrad && l + 1u < pol_u<kTable>(net.n_trunk)) pol_copy_tile(stash + (size_t)l * kPolTile, cur, t);
    }
    // the heads' hidden layers: each in a tile of its own when the backward pass needs them
    float *ha = kGrad ? s_pol + 2 * kPolTile : oth, *hc = kGrad ? s_pol + 3 * kPolTile : oth;
    pol_layer(pol_pick<kTable>(net.actor[0]), kActRelu, cur, ha, kPolStride, wv, 0u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.actor[1]), kActIdentity, ha, s_logit, kPolLogitStride, wv, 0u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.critic[0]), kActRelu, cur, hc, kPolStride, wv, 0u, lane);
    __syncthreads();
    pol_layer(pol_pick<kTable>(net.critic[1]), kActIdentity, hc, s_val, 1u, wv, 0u, lane);
    __syncthreads();

    // ---- one row per thread: logp, entropy, and d loss / d logits | d value
    // as the 16-column operands oth[:, 0:16] and oth[:, 16:32] (+0 pads) ----
    if (t < (uint32_t)kPolRows) {
        float dz[kPolActions] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, dv = 0.0f;
        if (t < nr) {
            const uint64_t r = r0 + t;
            float z[kPolActions];
#pragma unroll
            for (int i = 0; i < kPolActions; ++i) z[i] = s_logit[t * kPolLogitStride + i];
            const float gl = kGrad && A.g_logp ? A.g_logp[r] : 0.0f, ge = kGrad && A.g_entropy ? A.g_entropy[r] : 0.0f;
            float logp, ent;
            pol_head(z, A.action[r], gl, ge, &logp, &ent, dz);
            if (A.logp) A.logp[r] = logp;
            if (A.value) A.value[r] = s_val[t];
            if (A.entropy) A.entropy[r] = ent;
            if (kGrad && A.g_value) dv = A.g_value[r];
        }
        if (kGrad) {
            float *o = oth + t * kPolStride;
#pragma unroll
            for (int i = 0; i < 32; ++i) o[i] = 0.0f;
            if (t < nr) {
#pragma unroll
                for (int i = 0; i < kPolActions; ++i) o[i] = dz[i];
                o[16] = dv;
            }
        }
    }
    __syncthreads();
    if constexpr (kGrad) {
        const uint32_t T = pol_u<kTable>(net.n_trunk);
        // layer l's dW and db chains in the block's slab
        auto dw = [&](int l) { return slab + pol_u<kTable>(sw[l]); };
        auto db = [&](int l) { return slab + pol_u<kTable>(sb[l]); };
        // heads' second layers
        pol_grad_w(pol_pick<kTable>(net.actor[1]), oth, ha, dw(kPolMaxTrunk + 1), db(kPolMaxTrunk + 1), first, wv, lane, t);
        pol_grad_w(pol_pick<kTable>(net.critic[1]), oth + 16, hc, dw(kPolMaxTrunk + 3), db(kPolMaxTrunk + 3), first, wv,
                   lane, t);
        __syncthreads();
        pol_layer<true>(pol_pick<kTable>(back.actor[1]), kActRelu, oth, ha, kPolStride, wv, 0u, lane);
        pol_layer<true>(pol_pick<kTable>(back.critic[1]), kActRelu, oth + 16, hc, kPolStride, wv, 0u, lane);
        __syncthreads();
        // heads' first layers; the trunk's last output receives the actor's input
        // gradient plus the critic's, times its activation's derivative
        pol_grad_w(pol_pick<kTable>(net.actor[0]), ha, cur, dw(kPolMaxTrunk), db(kPolMaxTrunk), first, wv, lane, t);
        pol_grad_w(pol_pick<kTable>(net.critic[0]), hc, cur, dw(kPolMaxTrunk + 2), db(kPolMaxTrunk + 2), first, wv, lane,
                   t);
        pol_layer<true>(pol_pick<kTable>(back.actor[0]), -1, ha, oth, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer<true>(pol_pick<kTable>(back.critic[0]), (int)pol_u<kTable>(net.trunk[T - 1u].act), hc, cur, kPolStride,
                        wv, 0u, lane, oth);
        __syncthreads();
        // the trunk, last layer first: d in `cur`, the layer's input in `oth`
        for (uint32_t l = T; l-- > 0u;) {
            if (l == 0u) pol_stage_dense(oth, A, r0, nr, pol_u<kTable>(net.trunk[0].kp), mem_in, t);
            else pol_copy_tile(oth, stash + (size_t)(l - 1u) * kPolTile, t);
            __syncthreads();
            pol_grad_w(pol_pick<kTable>(net.trunk[l]), cur, oth, dw((int)l), db((int)l), first, wv, lane, t);
            __syncthreads();
            if (l == 0u) break;
            pol_layer<true>(pol_pick<kTable>(back.trunk[l]), (int)pol_u<kTable>(net.trunk[l - 1u].act), cur, oth,
                            kPolStride, wv, 0u, lane);
            __syncthreads();
            float *sw_ = cur;
            cur = oth;
            oth = sw_;
        }
    }
}

// kGrad false: every row, grid-stride over the tiles.  kGrad true: block b is
// accumulator b and takes the tiles b, b + kPolGradAcc, ... in order.
template <bool kGrad>
__global__ __launch_bounds__(256, kGrad ? 1 : 2) void policy_eval_kernel(PolEvalIO A, PolNet net, PolGradDev G)
{
    extern __shared__ float s_pol[];
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint64_t tiles = (A.n + kPolRows - 1u) / kPolRows;
    const uint64_t stride = kGrad ? (uint64_t)kPolGradAcc : (uint64_t)gridDim.x;
    float *slab = kGrad ? G.slabs.base + (size_t)blockIdx.x * G.slabs.slab_floats : nullptr;
    float *stash = kGrad ? G.stash + (size_t)blockIdx.x * kPolStashTiles * kPolTile : nullptr;

    for (uint64_t tile = blockIdx.x; tile < tiles; tile += stride) {
        const uint64_t r0 = tile * kPolRows;
        const uint32_t nr = A.n - r0 < (uint64_t)kPolRows ? (uint32_t)(A.n - r0) : (uint32_t)kPolRows;
        pol_eval_tile<kGrad, false>(A, net, G.back, G.slabs.w, G.slabs.b, slab, stash, r0, nr,
                                    tile == (uint64_t)blockIdx.x, s_pol, t, wv, lane);
    }
}

// layer `l`'s accumulators -- slabs [0, nacc) of `base`, `stride` floats apart,
// dW at `woff` in the C-fragment order, db at `boff` -- added in ascending index
// from +0 into the gradient's [out][in] / [out] layout (null: not wanted)
__device__ __forceinline__ void pol_reduce_layer(const float *base, uint64_t stride, uint32_t nacc, uint32_t woff,
                                                 uint32_t boff, uint32_t in, uint32_t out, uint32_t nkt, float *ow,
                                                 float *ob)
{
    const uint32_t nw = ow ? in * out : 0u, nb = ob ? out : 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nw + nb; i += gridDim.x * 256u) {
        size_t off;
        if (i < nw) {
            const uint32_t j = i / in, k = i - j * in;
            const uint32_t jt = j >> 4, q = (j & 15u) >> 2, r = j & 3u, kt = k >> 4, c = k & 15u;
            off = woff + ((size_t)(jt * nkt + kt) * 4u + r) * 64u + q * 16u + c;
        } else {
            off = boff + (i - nw);
        }
        float acc = 0.0f;
        for (uint32_t a = 0; a < nacc; ++a) acc = acc + base[(size_t)a * stride + off];
        if (i < nw) ow[i] = acc;
        else ob[i - nw] = acc;
    }
}

// the accumulators added in ascending index, each gradient in its [out][in] / [out] layout
__global__ __launch_bounds__(256) void policy_grad_reduce_kernel(PolGradSlabs S, PolGradOut O)
{
    const uint32_t l = blockIdx.y;
    pol_reduce_layer(S.base, S.slab_floats, S.nacc, S.w[l], S.b[l], O.in[l], O.out[l], pol_grad_nkt(O.kp[l]), O.w[l],
                     O.b[l]);
}

// ---- grouped evaluate (mbots_policy.hpp; DESIGN.md "Grouped evaluate") ----
// The descriptor table and the repack list of the nets [S.first, S.first +
// S.n), written from the launch's arguments: one thread per net.
__global__ __launch_bounds__(64) void policy_groups_setup_kernel(PolGroupSpecs S, float *ws, PolGroupEntry *table,
                                                                 PolUpload *uploads)
{
    const uint32_t i = threadIdx.x;
    if (i >= S.n) return;
    const uint32_t e = S.first + i;
    PolGroupEntry E;
    pol_group_entry(S.s[i], ws, E, uploads + (size_t)e * kPolGroupUploads);
    table[e] = E;
}

// every net's weights into the fragment orders: block (x, layer, net) of the
// repack list, gridDim.y entries per net (fwd_only: the transposed layers are
// not wanted)
__global__ __launch_bounds__(256) void policy_repack_groups_kernel(const PolUpload *uploads, uint32_t fwd_only)
{
    const PolUpload L = uploads[(size_t)blockIdx.z * gridDim.y + blockIdx.y];
    if (L.w_dst == nullptr || (fwd_only && L.tr)) return;
    pol_repack_layer(L);
}

__global__ __launch_bounds__(256) void policy_zero_rows_kernel(float *a, float *b, float *c, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        if (a) a[i] = 0.0f;
        if (b) b[i] = 0.0f;
        if (c) c[i] = 0.0f;
    }
}

// segment e's rows as the device reads them: hi as min(hi, n), lo as min(lo, hi)
// (and neither below 0)
__device__ __forceinline__ void pol_segment(const int32_t *segments, uint32_t e, uint64_t n, uint32_t &lo,
                                            uint32_t &len)
{
    const int32_t a = segments[2u * e], b = segments[2u * e + 1u];
    const uint32_t hi = (uint32_t)min((uint64_t)(b < 0 ? 0 : b), n);
    lo = min((uint32_t)(a < 0 ? 0 : a), hi);
    len = hi - lo;
}

// policy_act_groups_kernel's table behind evaluate's tile: first row, length and
// the inclusive scan of the tile counts of the (group, species) segments
constexpr size_t kPolEvalGroupLds = kPolEvalLds + (3u * kPolEvalMaxSegs + 4u) * sizeof(uint32_t);
static_assert(kPolEvalGroupLds <= 80u * 1024u, "two blocks of policy_eval_groups_kernel share a compute unit's LDS");
static_assert(kPolEvalMaxSegs == 256u, "policy_eval_groups_kernel: one segment entry per thread");

// logp, value and entropy of every row of every segment that has a net, grid-
// stride over the segments' tiles (a tile never straddles two segments)
__global__ __launch_bounds__(256, 2) void policy_eval_groups_kernel(PolEvalIO A, const int32_t *segments,
                                                                    const PolGroupEntry *table, uint32_t nseg)
{
    extern __shared__ float s_pol[];
    uint32_t *s_start = reinterpret_cast<uint32_t *>(s_pol) + kPolEvalLds / sizeof(uint32_t);
    uint32_t *s_len = s_start + kPolEvalMaxSegs, *s_scan = s_len + kPolEvalMaxSegs, *s_wsum = s_scan + kPolEvalMaxSegs;
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    {
        uint32_t lo = 0, len = 0;
        if (t < nseg && table[t].net.set) pol_segment(segments, t, A.n, lo, len);
        s_start[t] = lo;
        s_len[t] = len;
        uint32_t incl = (len + kPolRows - 1u) / kPolRows;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) s_wsum[wv] = incl;
        __syncthreads();
        for (uint32_t q = 0; q < wv; ++q) incl += s_wsum[q];
        s_scan[t] = incl;
        __syncthreads();
    }
    const uint32_t tiles = uniform(s_scan[kPolEvalMaxSegs - 1u]);

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // the first entry whose scan exceeds the tile (entries without rows are passed over)
        uint32_t lo = 0, hi = nseg - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_scan[mid] > tile) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t e = uniform(lo);
        const uint32_t rest = tile - (e ? uniform(s_scan[e - 1u]) : 0u);
        const uint32_t len = uniform(s_len[e]);
        const uint64_t r0 = (uint64_t)uniform(s_start[e]) + (uint64_t)rest * kPolRows;
        const uint32_t nr = min((uint32_t)kPolRows, len - rest * kPolRows);
        const PolGroupEntry &E = table[e];
        pol_eval_tile<false, true>(A, E.net, E.back, E.sw, E.sb, nullptr, nullptr, r0, nr, false, s_pol, t, wv, lane);
    }
}

// Block (a, c) is accumulator a of the wave's segment c: the tiles a, a +
// kPolGradAcc, ... counted from the segment's lo, into slab and stash (c, a).  A
// block without a tile leaves its slab alone: the reduce never reads it.
__global__ __launch_bounds__(256, 1) void policy_grad_groups_kernel(PolEvalIO A, const int32_t *segments,
                                                                    const PolGroupEntry *table, PolGroupWave Wv,
                                                                    float *slabs, uint64_t slab_stride, float *stash)
{
    extern __shared__ float s_pol[];
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint32_t a = blockIdx.x, c = blockIdx.y, e = Wv.seg[c];
    uint32_t lo, len;
    pol_segment(segments, e, A.n, lo, len);
    lo = uniform(lo);
    len = uniform(len);
    const uint32_t tiles = (len + kPolRows - 1u) / kPolRows;
    if (a >= tiles) return;
    const size_t blk = (size_t)c * gridDim.x + a;
    float *slab = slabs + blk * slab_stride;
    float *st = stash + blk * kPolStashTiles * kPolTile;
    const PolGroupEntry &E = table[e];
    for (uint32_t tile = a; tile < tiles; tile += kPolGradAcc) {
        const uint64_t r0 = (uint64_t)lo + (uint64_t)tile * kPolRows;
        const uint32_t nr = min((uint32_t)kPolRows, len - tile * kPolRows);
        pol_eval_tile<true, true>(A, E.net, E.back, E.sw, E.sb, slab, st, r0, nr, tile == a, s_pol, t, wv, lane);
    }
}

// block (x, layer, c): the wave's segment c adds the slabs its tiles reached,
// the first min(kPolGradAcc, tiles) -- none for an empty segment: zeros
__global__ __launch_bounds__(256) void policy_grad_groups_reduce_kernel(const int32_t *segments, uint64_t n,
                                                                        const PolGroupEntry *table, PolGroupWave Wv,
                                                                        PolGroupGrads O, const float *slabs,
                                                                        uint64_t slab_stride, uint32_t wave_acc)
{
    const uint32_t l = blockIdx.y, c = blockIdx.z, e = Wv.seg[c];
    const PolGroupEntry &E = table[e];
    if (l < (uint32_t)kPolMaxTrunk && l >= E.net.n_trunk) return;
    const uint32_t h = l - (uint32_t)kPolMaxTrunk;
    const PolLayer &f = l < (uint32_t)kPolMaxTrunk ? E.net.trunk[l] : h < 2u ? E.net.actor[h] : E.net.critic[h - 2u];
    uint32_t lo, len;
    pol_segment(segments, e, n, lo, len);
    const uint32_t nacc = min(min((len + kPolRows - 1u) / kPolRows, kPolGradAcc), wave_acc);
    pol_reduce_layer(slabs + (size_t)c * wave_acc * slab_stride, slab_stride, nacc, E.sw[l], E.sb[l], f.in, f.out,
                     pol_grad_nkt(f.kp), O.w[c][l], O.b[c][l]);
}

// ---- evaluate_sequences and its backward pass through time (mbots_policy.hpp;
// DESIGN.md "Backpropagation through HiddenState") ----
constexpr int kPolDmStride = 20;   // floats per row of the d mem_pre tile: 16 + 4, so the 16 rows x 4 k
                                   // of its A fragments hit 64 banks as the big tiles' do
constexpr int kPolHTile = kPolRows * kHidden;
constexpr size_t kPolSeqEvalLds = (2 * kPolTile + kPolRows * (kPolLogitStride + 1) + kPolHTile + kPolRows) * sizeof(float);
constexpr size_t kPolSeqGradLds =
    (4 * kPolTile + kPolRows * (kPolLogitStride + 1) + kPolHTile + 2 * kPolRows * kPolDmStride + kPolRows) *
    sizeof(float);

// A tile's columns.  kIndex false: the batch's own, b0 + row.  kIndex true: the
// entries idx[0 .. nb) of `order`, kept in s_col; an entry outside [0, B) (and
// every row past nb) is kPolNoColumn there -- a column of length 0 that is
// neither read nor written.
// element (k, row's column) of an [L][B] array; e0 = k B + b0
template <bool kIndex>
__device__ __forceinline__ uint64_t pol_seq_elem(const PolSeqIO &A, const uint32_t *s_col, uint32_t k, uint64_t e0,
                                                 uint32_t row)
{
    if constexpr (kIndex) return (uint64_t)k * A.B + s_col[row];
    else return e0 + row;
}
template <bool kIndex> __device__ __forceinline__ bool pol_seq_has_col(const uint32_t *s_col, uint32_t nb, uint32_t row)
{
    if constexpr (kIndex) return s_col[row] != kPolNoColumn;
    else return row < nb;
}

// the lengths of the tile's columns (clamped to [0, L]; 0 past B) into s_len, and the largest
template <bool kIndex>
__device__ __forceinline__ uint32_t pol_seq_lengths(uint32_t *s_len, uint32_t *s_col, const PolSeqIO &A,
                                                    const int32_t *idx, uint64_t b0, uint32_t nb, uint32_t t)
{
    __syncthreads();   // the previous tile's readers
    if (t < (uint32_t)kPolRows) {
        int32_t n = 0;
        if constexpr (kIndex) {
            uint32_t col = kPolNoColumn;
            if (t < nb) {
                const int32_t c = idx[t];
                if (c >= 0 && (uint64_t)c < A.B) {
                    col = (uint32_t)c;
                    n = A.length[col];
                }
            }
            s_col[t] = col;
        } else {
            n = t < nb ? A.length[b0 + t] : 0;
        }
        s_len[t] = n < 0 ? 0u : min((uint32_t)n, A.L);
    }
    __syncthreads();
    uint32_t m = 0;
    for (int r = 0; r < kPolRows; ++r) m = max(m, s_len[r]);
    return uniform(m);
}

// step k's inputs of the tile: X[64][kp] = obs[k, b0 + row] | h[row], +0 for the
// pads and the absent elements (h: [64][16], LDS or the block's store)
// (kIndex: a row's 69 obs floats lie at its own column, s_col[row]; they are
// contiguous whichever column that is.)
template <bool kIndex>
__device__ __forceinline__ void pol_stage_seq(float *x, const PolSeqIO &A, uint32_t k, uint64_t b0,
                                              const uint32_t *s_len, const uint32_t *s_col, const float *h, uint32_t kp,
                                              uint32_t t)
{
    const float *o = A.obs + ((uint64_t)k * A.B + b0) * kPolObs;
    for (uint32_t i = t; i < (uint32_t)kPolRows * kp; i += 256u) {
        const uint32_t row = i / kp, c = i - row * kp;
        float v = 0.0f;
        if (k < s_len[row]) {
            if (c < (uint32_t)kPolObs) {
                if constexpr (kIndex) v = A.obs[((uint64_t)k * A.B + s_col[row]) * kPolObs + c];
                else v = o[(size_t)row * kPolObs + c];
            } else if (c < (uint32_t)(kPolObs + kHidden)) v = h[row * kHidden + (c - kPolObs)];
        }
        x[row * kPolStride + c] = v;
    }
}

// One column tile of evaluate_sequences: logp, value, entropy (and the h_k read)
// of every element of its nb columns, k ascending with h carried in LDS.  kTable:
// `net` lies in device memory (the grouped call's descriptor table).  kIndex:
// the columns are idx[0 .. nb) (pol_seq_col), else b0 .. b0 + nb.
template <bool kTable, bool kIndex>
__device__ __forceinline__ void pol_seq_eval_tile(const PolSeqIO &A, const PolNet &net, const int32_t *idx, uint64_t b0,
                                                  uint32_t nb, float *s_pol, uint32_t t, uint32_t wv, uint32_t lane)
{
    float *buf0 = s_pol, *buf1 = s_pol + kPolTile;
    float *s_logit = s_pol + 2 * kPolTile, *s_val = s_logit + kPolRows * kPolLogitStride;
    float *s_h = s_val + kPolRows;
    uint32_t *s_len = reinterpret_cast<uint32_t *>(s_h + kPolHTile);
    uint32_t *s_col = s_len + kPolRows;   // (kIndex only)
    const uint32_t T = pol_u<kTable>(net.n_trunk), kp0 = pol_u<kTable>(net.trunk[0].kp);
    const bool gated = pol_u<kTable>(net.gated) != 0u;

    const uint32_t maxlen = pol_seq_lengths<kIndex>(s_len, s_col, A, idx, b0, nb, t);
    for (uint32_t i = t; i < (uint32_t)kPolHTile; i += 256u) {
        if constexpr (kIndex) {
            const uint32_t col = s_col[i >> 4];
            s_h[i] = col != kPolNoColumn ? A.hidden0[(uint64_t)col * kHidden + (i & 15u)] : 0.0f;
        } else {
            s_h[i] = (i >> 4) < nb ? A.hidden0[b0 * kHidden + i] : 0.0f;
        }
    }
    __syncthreads();
    for (uint32_t k = 0; k < maxlen; ++k) {
        const uint64_t e0 = (uint64_t)k * A.B + b0;
        if (A.hidden)
            for (uint32_t i = t; i < nb * (uint32_t)kHidden; i += 256u) {
                const float v = k < s_len[i >> 4] ? s_h[i] : 0.0f;
                if constexpr (kIndex) {
                    const uint32_t col = s_col[i >> 4];
                    if (col != kPolNoColumn) A.hidden[((uint64_t)k * A.B + col) * kHidden + (i & 15u)] = v;
                } else {
                    A.hidden[e0 * kHidden + i] = v;
                }
            }
        pol_stage_seq<kIndex>(buf0, A, k, b0, s_len, s_col, s_h, kp0, t);
        __syncthreads();
        float *cur = buf0, *oth = buf1;
        for (uint32_t l = 0; l < T; ++l) {
            pol_layer(pol_pick<kTable>(net.trunk[l]), (int)pol_u<kTable>(net.trunk[l].act), cur, oth, kPolStride, wv, 0u,
                      lane);
            __syncthreads();
            float *sw = cur;
            cur = oth;
            oth = sw;
        }
        pol_layer(pol_pick<kTable>(net.actor[0]), kActRelu, cur, oth, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.actor[1]), kActIdentity, oth, s_logit, kPolLogitStride, wv, 0u, lane);
        // h_{k+1}, as act() writes it (a gated net's: below)
        if (!gated) pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_h, kHidden, wv, 1u, lane);
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.critic[0]), kActRelu, cur, oth, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.critic[1]), kActIdentity, oth, s_val, 1u, wv, 0u, lane);
        __syncthreads();
        if (gated) {
            // c and z side by side in the tile the critic has done with (waves 0
            // and 1), then the blend with the h this step read
            float *s_c = oth, *s_z = oth + kPolHTile;
            const uint32_t gl = pol_opaque(lane);
            pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_c, kHidden, wv, 0u, gl);
            pol_layer<false, kPolStride, true>(pol_pick<kTable>(net.gate), kActSigmoid, cur, s_z, kHidden, wv, 1u, gl);
            __syncthreads();
            for (uint32_t i = wv * 64u + gl; i < (uint32_t)kPolHTile; i += 256u)
                s_h[i] = pol_gate_blend(s_z[i], s_c[i], s_h[i]);
            __syncthreads();   // the next step stages from s_h
        }
        if (t < nb && pol_seq_has_col<kIndex>(s_col, nb, t)) {
            const uint64_t e = pol_seq_elem<kIndex>(A, s_col, k, e0, t);
            float logp = 0.0f, ent = 0.0f, val = 0.0f;
            if (k < s_len[t]) {
                float z[kPolActions], dz[kPolActions];
#pragma unroll
                for (int i = 0; i < kPolActions; ++i) z[i] = s_logit[t * kPolLogitStride + i];
                pol_head(z, A.action[e], 0.0f, 0.0f, &logp, &ent, dz);
                val = s_val[t];
            }
            if (A.logp) A.logp[e] = logp;
            if (A.value) A.value[e] = val;
            if (A.entropy) A.entropy[e] = ent;
        }
    }
    // the steps past the tile's largest length
    for (uint32_t k = maxlen; k < A.L; ++k) {
        const uint64_t e0 = (uint64_t)k * A.B + b0;
        if (t < nb && pol_seq_has_col<kIndex>(s_col, nb, t)) {
            const uint64_t e = pol_seq_elem<kIndex>(A, s_col, k, e0, t);
            if (A.logp) A.logp[e] = 0.0f;
            if (A.value) A.value[e] = 0.0f;
            if (A.entropy) A.entropy[e] = 0.0f;
        }
        if (A.hidden)
            for (uint32_t i = t; i < nb * (uint32_t)kHidden; i += 256u) {
                if constexpr (kIndex) {
                    const uint32_t col = s_col[i >> 4];
                    if (col != kPolNoColumn) A.hidden[((uint64_t)k * A.B + col) * kHidden + (i & 15u)] = 0.0f;
                } else {
                    A.hidden[e0 * kHidden + i] = 0.0f;
                }
            }
    }
}

// every column of the batch through one net, grid-stride over the column tiles
__global__ __launch_bounds__(256, 2) void policy_seq_eval_kernel(PolSeqIO A, PolNet net)
{
    extern __shared__ float s_pol[];
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint64_t tiles = (A.B + kPolRows - 1u) / kPolRows;

    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t b0 = tile * kPolRows;
        const uint32_t nb = A.B - b0 < (uint64_t)kPolRows ? (uint32_t)(A.B - b0) : (uint32_t)kPolRows;
        pol_seq_eval_tile<false, false>(A, net, nullptr, b0, nb, s_pol, t, wv, lane);
    }
}

struct PolSeqGradDev {
    PolNet back;          // the transposed layers; memory the head's, trunk[0] the H -> 16 layer of dh
    PolGradSlabs slabs;
    float *stash;         // [blocks][kPolStashTiles][kPolTile]
    float *hws;           // [blocks][L][64][16]
};

// One column tile of evaluate_sequences' backward pass, continuing the chains
// of the block's slab (`started`: they have begun; returns whether they have
// now): a forward sweep that keeps
// only h_k (in the block's store hk, [L][64][16]); then for k descending that
// step's forward again from (obs_k, h_k), and policy_eval_kernel's backward with
// the memory head's gradients (slot kPolGradLayers), d mem_pre from the carried
// dh tile, and the next dh from the first layer's gradient (back.trunk[0], the
// H -> 16 layer over W0[:, 69:85]).  kTable, kIndex, idx, b0: as
// pol_seq_eval_tile; layer l's dW at sw[l], db at sb[l] of the slab.
template <bool kTable, bool kIndex>
__device__ __forceinline__ bool pol_seq_grad_tile(const PolSeqIO &A, const PolNet &net, const PolNet &back,
                                                  const uint32_t *sw, const uint32_t *sb, float *slab, float *stash,
                                                  float *hk, const int32_t *idx, uint64_t b0, uint32_t nb, bool started,
                                                  float *s_pol, uint32_t t, uint32_t wv, uint32_t lane)
{
    float *buf0 = s_pol, *buf1 = s_pol + kPolTile, *ha = s_pol + 2 * kPolTile, *hc = s_pol + 3 * kPolTile;
    float *s_logit = s_pol + 4 * kPolTile, *s_val = s_logit + kPolRows * kPolLogitStride;
    float *s_hd = s_val + kPolRows;        // h during the sweep, dh on the way back
    float *s_dm = s_hd + kPolHTile;        // the memory head's output y, then d mem_pre
    float *s_dg = s_dm + kPolRows * kPolDmStride;   // (gated) the gate's output z, then d gate_pre
    uint32_t *s_len = reinterpret_cast<uint32_t *>(s_dg + kPolRows * kPolDmStride);
    uint32_t *s_col = s_len + kPolRows;    // (kIndex only)
    const uint32_t T = pol_u<kTable>(net.n_trunk), kp0 = pol_u<kTable>(net.trunk[0].kp);
    const bool gated = pol_u<kTable>(net.gated) != 0u;
    constexpr int kM = kPolGradLayers;   // the memory head's slot
    constexpr int kG = kPolSeqLayers;    // the gate head's
    auto dw = [&](int l) { return slab + pol_u<kTable>(sw[l]); };
    auto db = [&](int l) { return slab + pol_u<kTable>(sb[l]); };

    const uint32_t maxlen = pol_seq_lengths<kIndex>(s_len, s_col, A, idx, b0, nb, t);
    // ---- the forward sweep: h_k of every step ----
    for (uint32_t i = t; i < (uint32_t)kPolHTile; i += 256u) {
        if constexpr (kIndex) {
            const uint32_t col = s_col[i >> 4];
            s_hd[i] = col != kPolNoColumn ? A.hidden0[(uint64_t)col * kHidden + (i & 15u)] : 0.0f;
        } else {
            s_hd[i] = (i >> 4) < nb ? A.hidden0[b0 * kHidden + i] : 0.0f;
        }
    }
    __syncthreads();
    for (uint32_t k = 0; k < maxlen; ++k) {
        for (uint32_t i = t; i < (uint32_t)kPolHTile; i += 256u) hk[(size_t)k * kPolHTile + i] = s_hd[i];
        if (k + 1u == maxlen) break;
        pol_stage_seq<kIndex>(buf0, A, k, b0, s_len, s_col, s_hd, kp0, t);
        __syncthreads();
        float *cur = buf0, *oth = buf1;
        for (uint32_t l = 0; l < T; ++l) {
            pol_layer(pol_pick<kTable>(net.trunk[l]), (int)pol_u<kTable>(net.trunk[l].act), cur, oth, kPolStride, wv, 0u,
                      lane);
            __syncthreads();
            float *sw_ = cur;
            cur = oth;
            oth = sw_;
        }
        if (!gated) {
            pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_hd, kHidden, wv, 0u, lane);
        } else {
            const uint32_t gl = pol_opaque(lane);
            pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_dm, kPolDmStride, wv, 0u, gl);
            pol_layer<false, kPolStride, true>(pol_pick<kTable>(net.gate), kActSigmoid, cur, s_dg, kPolDmStride, wv, 1u,
                                               gl);
            __syncthreads();
            for (uint32_t i = wv * 64u + gl; i < (uint32_t)kPolHTile; i += 256u) {
                const uint32_t d = (i >> 4) * kPolDmStride + (i & 15u);
                s_hd[i] = pol_gate_blend(s_dg[d], s_dm[d], s_hd[i]);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t i = t; i < (uint32_t)kPolHTile; i += 256u) s_hd[i] = 0.0f;   // dh past the last step
    // ---- backward in time ----
    for (uint32_t k = maxlen; k-- > 0u;) {
        const float *h = hk + (size_t)k * kPolHTile;
        const uint64_t e0 = (uint64_t)k * A.B + b0;
        const bool first = !started;
        pol_stage_seq<kIndex>(buf0, A, k, b0, s_len, s_col, h, kp0, t);
        __syncthreads();
        float *cur = buf0, *oth = buf1;
        for (uint32_t l = 0; l < T; ++l) {
            pol_layer(pol_pick<kTable>(net.trunk[l]), (int)pol_u<kTable>(net.trunk[l].act), cur, oth, kPolStride, wv, 0u,
                      lane);
            __syncthreads();
            float *sw_ = cur;
            cur = oth;
            oth = sw_;
            if (l + 1u < T) pol_copy_tile(stash + (size_t)l * kPolTile, cur, t);
        }
        pol_layer(pol_pick<kTable>(net.actor[0]), kActRelu, cur, ha, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.actor[1]), kActIdentity, ha, s_logit, kPolLogitStride, wv, 0u, lane);
        pol_layer(pol_pick<kTable>(net.memory), kActTanh, cur, s_dm, kPolDmStride, wv, 1u, lane);
        if (gated)
            pol_layer<false, kPolStride, true>(pol_pick<kTable>(net.gate), kActSigmoid, cur, s_dg, kPolDmStride, wv, 2u,
                                               pol_opaque(lane));
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.critic[0]), kActRelu, cur, hc, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer(pol_pick<kTable>(net.critic[1]), kActIdentity, hc, s_val, 1u, wv, 0u, lane);
        __syncthreads();
        // d loss / d logits | d value as in policy_eval_kernel, and d mem_pre = dh (1 - y^2)
        if (t < (uint32_t)kPolRows) {
            float dz[kPolActions] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, dv = 0.0f;
            const bool present = k < s_len[t];
            if (present) {
                const uint64_t e = pol_seq_elem<kIndex>(A, s_col, k, e0, t);
                float z[kPolActions];
#pragma unroll
                for (int i = 0; i < kPolActions; ++i) z[i] = s_logit[t * kPolLogitStride + i];
                const float gl = A.g_logp ? A.g_logp[e] : 0.0f, ge = A.g_entropy ? A.g_entropy[e] : 0.0f;
                float logp, ent;
                pol_head(z, A.action[e], gl, ge, &logp, &ent, dz);
                if (A.g_value) dv = A.g_value[e];
            }
            float *o = oth + t * kPolStride;
#pragma unroll
            for (int i = 0; i < 32; ++i) o[i] = 0.0f;
            if (present) {
#pragma unroll
                for (int i = 0; i < kPolActions; ++i) o[i] = dz[i];
                o[16] = dv;
            }
        }
        {
            const uint32_t row = t >> 2, c0 = (t & 3u) * 4u;
            const bool present = k < s_len[row];
            if (!gated) {
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    float *y = s_dm + row * kPolDmStride + c0 + u;
                    *y = present ? s_hd[row * kHidden + c0 + u] * pol_activation_grad(kActTanh, *y) : 0.0f;
                }
            } else {
                // d mem_pre, d gate_pre, and in place of dh_{k+1} its direct term dh (1 - z)
                const uint32_t e0_ = pol_opaque(row * kPolDmStride + c0), h0_ = pol_opaque(row * kHidden + c0);
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    float *y = s_dm + e0_ + u, *z = s_dg + e0_ + u;
                    float *d = s_hd + h0_ + u;
                    float dc = 0.0f, dg = 0.0f, dd = 0.0f;
                    if (present) pol_gate_back(*d, *z, *y, h[h0_ + u], &dc, &dg, &dd);
                    *y = dc;
                    *z = dg;
                    *d = dd;
                }
            }
        }
        __syncthreads();
        // heads' second layers, and the memory head
        pol_grad_w(pol_pick<kTable>(net.actor[1]), oth, ha, dw(kPolMaxTrunk + 1), db(kPolMaxTrunk + 1), first, wv, lane, t);
        pol_grad_w(pol_pick<kTable>(net.critic[1]), oth + 16, hc, dw(kPolMaxTrunk + 3), db(kPolMaxTrunk + 3), first, wv,
                   lane, t);
        pol_grad_w<kPolDmStride>(pol_pick<kTable>(net.memory), s_dm, cur, dw(kM), db(kM), first, wv, lane, t);
        if (gated) {
            const uint32_t gl = pol_opaque(lane);
            pol_grad_w<kPolDmStride>(pol_pick<kTable>(net.gate), s_dg, cur, dw(kG), db(kG), first, wv, gl, wv * 64u + gl);
        }
        __syncthreads();
        pol_layer<true>(pol_pick<kTable>(back.actor[1]), kActRelu, oth, ha, kPolStride, wv, 0u, lane);
        pol_layer<true>(pol_pick<kTable>(back.critic[1]), kActRelu, oth + 16, hc, kPolStride, wv, 0u, lane);
        __syncthreads();
        // heads' first layers; the trunk's last output receives the actor's input
        // gradient, plus the critic's, plus the memory head's, times its
        // activation's derivative
        pol_grad_w(pol_pick<kTable>(net.actor[0]), ha, cur, dw(kPolMaxTrunk), db(kPolMaxTrunk), first, wv, lane, t);
        pol_grad_w(pol_pick<kTable>(net.critic[0]), hc, cur, dw(kPolMaxTrunk + 2), db(kPolMaxTrunk + 2), first, wv, lane,
                   t);
        pol_layer<true>(pol_pick<kTable>(back.actor[0]), -1, ha, oth, kPolStride, wv, 0u, lane);
        __syncthreads();
        pol_layer<true>(pol_pick<kTable>(back.critic[0]), -1, hc, oth, kPolStride, wv, 0u, lane, oth);
        __syncthreads();
        if (!gated) {
            pol_layer<true, kPolDmStride>(pol_pick<kTable>(back.memory), (int)pol_u<kTable>(net.trunk[T - 1u].act), s_dm,
                                          cur, kPolStride, wv, 0u, lane, oth);
        } else {   // ... plus the gate's, joined last
            const uint32_t gl = pol_opaque(lane);
            pol_layer<true, kPolDmStride>(pol_pick<kTable>(back.memory), -1, s_dm, oth, kPolStride, wv, 0u, gl, oth);
            __syncthreads();
            pol_layer<true, kPolDmStride>(pol_pick<kTable>(back.gate), (int)pol_u<kTable>(net.trunk[T - 1u].act), s_dg,
                                          cur, kPolStride, wv, 0u, gl, oth);
        }
        __syncthreads();
        // the trunk, last layer first: d in `cur`, the layer's input in `oth`
        for (uint32_t l = T; l-- > 0u;) {
            if (l == 0u) pol_stage_seq<kIndex>(oth, A, k, b0, s_len, s_col, h, kp0, t);
            else pol_copy_tile(oth, stash + (size_t)(l - 1u) * kPolTile, t);
            __syncthreads();
            pol_grad_w(pol_pick<kTable>(net.trunk[l]), cur, oth, dw((int)l), db((int)l), first, wv, lane, t);
            __syncthreads();
            if (l == 0u) break;
            pol_layer<true>(pol_pick<kTable>(back.trunk[l]), (int)pol_u<kTable>(net.trunk[l - 1u].act), cur, oth,
                            kPolStride, wv, 0u, lane);
            __syncthreads();
            float *sw_ = cur;
            cur = oth;
            oth = sw_;
        }
        // dh_k[c] = sum_j d0[j] W0[j][69 + c] (gated: added to the direct term s_hd holds)
        if (!gated) pol_layer<true>(pol_pick<kTable>(back.trunk[0]), -1, cur, s_hd, kHidden, wv, 0u, lane);
        else pol_layer<true>(pol_pick<kTable>(back.trunk[0]), -1, cur, s_hd, kHidden, wv, 0u, pol_opaque(lane), s_hd);
        __syncthreads();
        started = true;
    }
    return started;
}

// Block b is accumulator b and takes the column tiles b, b + kPolGradAcc, ...
// in order.
__global__ __launch_bounds__(256, 1) void policy_seq_grad_kernel(PolSeqIO A, PolNet net, PolSeqGradDev G)
{
    extern __shared__ float s_pol[];
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint64_t tiles = (A.B + kPolRows - 1u) / kPolRows;
    const PolGradSlabs &S = G.slabs;
    float *slab = S.base + (size_t)blockIdx.x * S.slab_floats;
    float *stash = G.stash + (size_t)blockIdx.x * kPolStashTiles * kPolTile;
    float *hk = G.hws + (size_t)blockIdx.x * A.L * kPolHTile;
    bool started = false;                // the slab's chains have begun

    for (uint64_t tile = blockIdx.x; tile < tiles; tile += (uint64_t)kPolGradAcc) {
        const uint64_t b0 = tile * kPolRows;
        const uint32_t nb = A.B - b0 < (uint64_t)kPolRows ? (uint32_t)(A.B - b0) : (uint32_t)kPolRows;
        started = pol_seq_grad_tile<false, false>(A, net, G.back, S.w, S.b, slab, stash, hk, nullptr, b0, nb, started,
                                                  s_pol, t, wv, lane);
    }
    if (!started)   // no step at all: the chains are their +0 starts
        for (size_t i = t; i < S.slab_floats; i += 256u) slab[i] = 0.0f;
}

// ---- grouped evaluate_sequences (mbots_policy.hpp; DESIGN.md "Grouped
// evaluate_sequences") ----
// the seq nets [S.first, S.first + S.n) into the descriptor table and the repack list
__global__ __launch_bounds__(64) void policy_seq_groups_setup_kernel(PolSeqGroupSpecs S, float *ws, PolGroupEntry *table,
                                                                     PolUpload *uploads)
{
    const uint32_t i = threadIdx.x;
    if (i >= S.n) return;
    const uint32_t e = S.first + i;
    PolGroupEntry E;
    pol_group_entry(S.s[i].s, ws, E, uploads + (size_t)e * kPolSeqGroupUploads, kPolSeqGroupUploads, true, S.s[i].mw,
                    S.s[i].mb, S.s[i].gw, S.s[i].gb);
    table[e] = E;
}

// the segment table of policy_eval_groups_kernel behind evaluate_sequences' tile
// and the tile's 64 column indices
constexpr size_t kPolSeqEvalTileLds = kPolSeqEvalLds + kPolRows * sizeof(uint32_t);
constexpr size_t kPolSeqEvalGroupLds = kPolSeqEvalTileLds + (3u * kPolEvalMaxSegs + 4u) * sizeof(uint32_t);
constexpr size_t kPolSeqGradGroupLds = kPolSeqGradLds + kPolRows * sizeof(uint32_t);
static_assert(kPolSeqEvalGroupLds <= 80u * 1024u, "two blocks of policy_seq_eval_groups_kernel share a compute unit's LDS");
static_assert(kPolSeqGradGroupLds <= 160u * 1024u, "a block of policy_seq_grad_groups_kernel fits a compute unit's LDS");

// logp, value, entropy (and h_k) of every column of every segment that has a
// net, grid-stride over the segments' tiles of 64 positions of `order` (a tile
// never straddles two segments)
__global__ __launch_bounds__(256, 2) void policy_seq_eval_groups_kernel(PolSeqIO A, const int32_t *order,
                                                                        const int32_t *segments,
                                                                        const PolGroupEntry *table, uint32_t nseg)
{
    extern __shared__ float s_pol[];
    uint32_t *s_start = reinterpret_cast<uint32_t *>(s_pol) + kPolSeqEvalTileLds / sizeof(uint32_t);
    uint32_t *s_len = s_start + kPolEvalMaxSegs, *s_scan = s_len + kPolEvalMaxSegs, *s_wsum = s_scan + kPolEvalMaxSegs;
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    {
        uint32_t lo = 0, len = 0;
        if (t < nseg && table[t].net.set) pol_segment(segments, t, A.B, lo, len);
        s_start[t] = lo;
        s_len[t] = len;
        uint32_t incl = (len + kPolRows - 1u) / kPolRows;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) s_wsum[wv] = incl;
        __syncthreads();
        for (uint32_t q = 0; q < wv; ++q) incl += s_wsum[q];
        s_scan[t] = incl;
        __syncthreads();
    }
    const uint32_t tiles = uniform(s_scan[kPolEvalMaxSegs - 1u]);

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t lo = 0, hi = nseg - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_scan[mid] > tile) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t e = uniform(lo);
        const uint32_t rest = tile - (e ? uniform(s_scan[e - 1u]) : 0u);
        const uint32_t len = uniform(s_len[e]);
        const uint32_t p0 = uniform(s_start[e]) + rest * kPolRows;
        const uint32_t nb = min((uint32_t)kPolRows, len - rest * kPolRows);
        pol_seq_eval_tile<true, true>(A, table[e].net, order + p0, 0u, nb, s_pol, t, wv, lane);
    }
}

// Block (a, c) is accumulator a of the wave's segment c: the tiles a, a +
// kPolGradAcc, ... of the segment's positions, into slab, stash and h store (c,
// a).  A block without a tile leaves its slab alone: the reduce never reads it.
__global__ __launch_bounds__(256, 1) void policy_seq_grad_groups_kernel(PolSeqIO A, const int32_t *order,
                                                                        const int32_t *segments,
                                                                        const PolGroupEntry *table, PolGroupWave Wv,
                                                                        float *slabs, uint64_t slab_stride, float *stash,
                                                                        float *hws)
{
    extern __shared__ float s_pol[];
    const uint32_t t = threadIdx.x, wv = uniform(t >> 6), lane = t & 63u;
    const uint32_t a = blockIdx.x, c = blockIdx.y, e = Wv.seg[c];
    uint32_t lo, len;
    pol_segment(segments, e, A.B, lo, len);
    lo = uniform(lo);
    len = uniform(len);
    const uint32_t tiles = (len + kPolRows - 1u) / kPolRows;
    if (a >= tiles) return;
    const size_t blk = (size_t)c * gridDim.x + a;
    float *slab = slabs + blk * slab_stride;
    float *st = stash + blk * kPolStashTiles * kPolTile;
    float *hk = hws + blk * A.L * kPolHTile;
    const PolGroupEntry &E = table[e];
    bool started = false;
    for (uint32_t tile = a; tile < tiles; tile += kPolGradAcc) {
        const uint32_t nb = min((uint32_t)kPolRows, len - tile * kPolRows);
        started = pol_seq_grad_tile<true, true>(A, E.net, E.back, E.sw, E.sb, slab, st, hk,
                                                order + lo + tile * kPolRows, 0u, nb, started, s_pol, t, wv, lane);
    }
    if (!started) {   // tiles without a step: the chains are their +0 starts
        const uint32_t n = uniform(E.slab_floats);
        for (uint32_t i = t; i < n; i += 256u) slab[i] = 0.0f;
    }
}

// block (x, layer, c): policy_grad_groups_reduce_kernel with the memory head's slot
__global__ __launch_bounds__(256) void policy_seq_grad_groups_reduce_kernel(const int32_t *segments, uint64_t n,
                                                                            const PolGroupEntry *table, PolGroupWave Wv,
                                                                            PolSeqGroupGrads O, const float *slabs,
                                                                            uint64_t slab_stride, uint32_t wave_acc)
{
    const uint32_t l = blockIdx.y, c = blockIdx.z, e = Wv.seg[c];
    const PolGroupEntry &E = table[e];
    if (l < (uint32_t)kPolMaxTrunk && l >= E.net.n_trunk) return;
    if (l == (uint32_t)kPolSeqLayers && !E.net.gated) return;
    const uint32_t h = l - (uint32_t)kPolMaxTrunk;
    const PolLayer &f = l < (uint32_t)kPolMaxTrunk ? E.net.trunk[l]
                        : h < 2u                   ? E.net.actor[h]
                        : h < 4u                   ? E.net.critic[h - 2u]
                        : h < 5u                   ? E.net.memory
                                                   : E.net.gate;
    uint32_t lo, len;
    pol_segment(segments, e, n, lo, len);
    const uint32_t nacc = min(min((len + kPolRows - 1u) / kPolRows, kPolGradAcc), wave_acc);
    pol_reduce_layer(slabs + (size_t)c * wave_acc * slab_stride, slab_stride, nacc, E.sw[l], E.sb[l], f.in, f.out,
                     pol_grad_nkt(f.kp), O.w[c][l], O.b[c][l]);
}

// ---- sequence_segments: a stable counting sort of the columns by net_id, at
// most 256 keys.  Chunks of kPolOrderChunk columns, one block each; thread k is
// key k throughout, and walks its chunk in column order, so no atomic and no
// race decides a position. ----
constexpr uint32_t kPolOrderChunk = 1024;

// counts[chunk][key]
__global__ __launch_bounds__(256) void policy_seq_order_count_kernel(const int32_t *net_id, uint64_t B, uint32_t *counts)
{
    __shared__ int32_t s_id[kPolOrderChunk];
    const uint64_t c0 = (uint64_t)blockIdx.x * kPolOrderChunk;
    const uint32_t n = (uint32_t)min((uint64_t)kPolOrderChunk, B - c0);
    for (uint32_t i = threadIdx.x; i < n; i += 256u) s_id[i] = net_id[c0 + i];
    __syncthreads();
    const int32_t key = (int32_t)threadIdx.x;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < n; ++i) cnt += s_id[i] == key ? 1u : 0u;
    counts[(size_t)blockIdx.x * 256u + threadIdx.x] = cnt;
}

// one block: counts[chunk][key] becomes the position of the chunk's first
// column of the key; segments[key] = [lo, hi); counts[nchunks][0] the total
__global__ __launch_bounds__(256) void policy_seq_order_scan_kernel(uint32_t *counts, uint32_t nchunks, uint32_t nkeys,
                                                                    int32_t *segments)
{
    __shared__ uint32_t s_tot[256];
    const uint32_t key = threadIdx.x;
    uint32_t tot = 0;
    if (key < nkeys)
        for (uint32_t c = 0; c < nchunks; ++c) tot += counts[(size_t)c * 256u + key];
    s_tot[key] = tot;
    __syncthreads();
    uint32_t lo = 0;
    for (uint32_t q = 0; q < key; ++q) lo += s_tot[q];
    if (key < nkeys) {
        segments[2u * key] = (int32_t)lo;
        segments[2u * key + 1u] = (int32_t)(lo + tot);
        uint32_t run = lo;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t n = counts[(size_t)c * 256u + key];
            counts[(size_t)c * 256u + key] = run;
            run += n;
        }
    }
    if (key == 255u) counts[(size_t)nchunks * 256u] = lo + tot;
}

// order[position] = column, each chunk's columns of a key ascending from the
// chunk's base; the tail past the last segment -1
__global__ __launch_bounds__(256) void policy_seq_order_scatter_kernel(const int32_t *net_id, uint64_t B,
                                                                       const uint32_t *counts, uint32_t nchunks,
                                                                       uint32_t nkeys, int32_t *order)
{
    __shared__ int32_t s_id[kPolOrderChunk];
    const uint64_t c0 = (uint64_t)blockIdx.x * kPolOrderChunk;
    const uint32_t n = (uint32_t)min((uint64_t)kPolOrderChunk, B - c0);
    for (uint32_t i = threadIdx.x; i < n; i += 256u) s_id[i] = net_id[c0 + i];
    __syncthreads();
    const uint32_t key = threadIdx.x;
    if (key < nkeys) {
        uint64_t p = counts[(size_t)blockIdx.x * 256u + key];
        for (uint32_t i = 0; i < n; ++i)
            if (s_id[i] == (int32_t)key && p < B) order[p++] = (int32_t)(c0 + i);
    }
    const uint64_t total = counts[(size_t)nchunks * 256u];
    for (uint64_t p = total + c0 + threadIdx.x; p < min(B, total + c0 + kPolOrderChunk); p += 256u) order[p] = -1;
}

template <bool kGrad> static hipError_t policy_eval_lds()
{
    static bool set = false;
    if (set) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(policy_eval_kernel<kGrad>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kGrad ? kPolGradLds : kPolEvalLds));
    if (e == hipSuccess) set = true;
    return e;
}

hipError_t launch_policy_eval(const PolEvalIO &io, const PolNet &net, hipStream_t st)
{
    if (io.n == 0) return hipSuccess;
    if (const hipError_t e = policy_eval_lds<false>()) return e;
    const uint64_t tiles = (io.n + kPolRows - 1u) / kPolRows;
    const unsigned blocks = (unsigned)std::min<uint64_t>(tiles, 512u);
    hipLaunchKernelGGL(policy_eval_kernel<false>, dim3(blocks), dim3(256), kPolEvalLds, st, io, net, PolGradDev{});
    return hipGetLastError();
}

size_t policy_grad_stash_floats(uint32_t nacc) { return (size_t)nacc * kPolStashTiles * kPolTile; }

hipError_t launch_policy_grad(const PolEvalIO &io, const PolNet &net, const PolNet &back, const PolGradSlabs &slabs,
                              float *stash, const PolGradOut &out, hipStream_t st)
{
    if (slabs.nacc) {
        if (const hipError_t e = policy_eval_lds<true>()) return e;
        PolGradDev G{back, slabs, stash};
        hipLaunchKernelGGL(policy_eval_kernel<true>, dim3(slabs.nacc), dim3(256), kPolGradLds, st, io, net, G);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_grad_reduce_kernel, dim3(16, out.n), dim3(256), 0, st, slabs, out);
    return hipGetLastError();
}

static hipError_t policy_seq_lds(const void *fn, size_t bytes, bool &set)
{
    if (set) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) set = true;
    return e;
}

// ---- grouped evaluate: the descriptor table and the repacked weights of the
// 4 G nets of `specs` (host memory: they travel as kernel arguments), then the
// forward, or the backward in waves of kPolGroupWave segments ----
static hipError_t policy_groups_prepare(const PolGroupSpec *specs, uint32_t nseg, float *ws, PolGroupEntry *table,
                                        PolUpload *uploads, bool fwd_only, hipStream_t st)
{
    for (uint32_t first = 0; first < nseg; first += kPolGroupChunk) {
        PolGroupSpecs S{};
        S.first = first;
        S.n = std::min(kPolGroupChunk, nseg - first);
        std::copy(specs + first, specs + first + S.n, S.s);
        hipLaunchKernelGGL(policy_groups_setup_kernel, dim3(1), dim3(64), 0, st, S, ws, table, uploads);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_repack_groups_kernel, dim3(8, kPolGroupUploads, nseg), dim3(256), 0, st, uploads,
                       fwd_only ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_policy_eval_groups(const PolEvalIO &io, const int32_t *segments, const PolGroupSpec *specs,
                                     uint32_t nseg, float *ws, PolGroupEntry *table, PolUpload *uploads, hipStream_t st)
{
    if (io.n == 0) return hipSuccess;
    static bool set = false;
    if (const hipError_t e =
            policy_seq_lds(reinterpret_cast<const void *>(policy_eval_groups_kernel), kPolEvalGroupLds, set))
        return e;
    if (const hipError_t e = policy_groups_prepare(specs, nseg, ws, table, uploads, true, st)) return e;
    const unsigned zb = (unsigned)std::min<uint64_t>((io.n + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(policy_zero_rows_kernel, dim3(zb), dim3(256), 0, st, io.logp, io.value, io.entropy, io.n);
    if (const hipError_t e = hipGetLastError()) return e;
    // never more blocks than the rows can hold tiles (each segment with a ragged one)
    const unsigned blocks = (unsigned)std::min<uint64_t>(io.n / kPolRows + nseg, 512u);
    hipLaunchKernelGGL(policy_eval_groups_kernel, dim3(blocks), dim3(256), kPolEvalGroupLds, st, io, segments, table,
                       nseg);
    return hipGetLastError();
}

hipError_t launch_policy_grad_groups(const PolEvalIO &io, const int32_t *segments, const PolGroupSpec *specs,
                                     uint32_t nseg, const PolGroupWave *waves, const PolGroupGrads *grads,
                                     uint32_t nwaves, float *ws, PolGroupEntry *table, PolUpload *uploads, float *slabs,
                                     uint64_t slab_stride, float *stash, uint32_t wave_acc, hipStream_t st)
{
    static bool set = false;
    if (const hipError_t e =
            policy_seq_lds(reinterpret_cast<const void *>(policy_grad_groups_kernel), kPolGradLds, set))
        return e;
    if (const hipError_t e = policy_groups_prepare(specs, nseg, ws, table, uploads, false, st)) return e;
    for (uint32_t w = 0; w < nwaves; ++w) {
        if (wave_acc) {
            hipLaunchKernelGGL(policy_grad_groups_kernel, dim3(wave_acc, waves[w].n), dim3(256), kPolGradLds, st, io,
                               segments, table, waves[w], slabs, slab_stride, stash);
            if (const hipError_t e = hipGetLastError()) return e;
        }
        hipLaunchKernelGGL(policy_grad_groups_reduce_kernel, dim3(16, kPolGradLayers, waves[w].n), dim3(256), 0, st,
                           segments, io.n, table, waves[w], grads[w], slabs, slab_stride, wave_acc);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// ---- grouped evaluate_sequences: policy_groups_prepare for nets with a memory
// head, then the zeroed outputs and the forward, or the backward in waves ----
static hipError_t policy_seq_groups_prepare(const PolSeqGroupSpec *specs, uint32_t nseg, float *ws, PolGroupEntry *table,
                                            PolUpload *uploads, bool fwd_only, hipStream_t st)
{
    for (uint32_t first = 0; first < nseg; first += kPolSeqGroupChunk) {
        PolSeqGroupSpecs S{};
        S.first = first;
        S.n = std::min(kPolSeqGroupChunk, nseg - first);
        std::copy(specs + first, specs + first + S.n, S.s);
        hipLaunchKernelGGL(policy_seq_groups_setup_kernel, dim3(1), dim3(64), 0, st, S, ws, table, uploads);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_repack_groups_kernel, dim3(8, kPolSeqGroupUploads, nseg), dim3(256), 0, st, uploads,
                       fwd_only ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_policy_seq_eval_groups(const PolSeqIO &io, const int32_t *order, const int32_t *segments,
                                         const PolSeqGroupSpec *specs, uint32_t nseg, float *ws, PolGroupEntry *table,
                                         PolUpload *uploads, hipStream_t st)
{
    if (io.B == 0 || io.L == 0) return hipSuccess;
    static bool set = false;
    if (const hipError_t e =
            policy_seq_lds(reinterpret_cast<const void *>(policy_seq_eval_groups_kernel), kPolSeqEvalGroupLds, set))
        return e;
    if (const hipError_t e = policy_seq_groups_prepare(specs, nseg, ws, table, uploads, true, st)) return e;
    const uint64_t n = (uint64_t)io.L * io.B;
    hipLaunchKernelGGL(policy_zero_rows_kernel, dim3((unsigned)std::min<uint64_t>((n + 255u) / 256u, 2048u)), dim3(256), 0,
                       st, io.logp, io.value, io.entropy, n);
    if (const hipError_t e = hipGetLastError()) return e;
    if (io.hidden) {
        hipLaunchKernelGGL(policy_zero_rows_kernel, dim3((unsigned)std::min<uint64_t>((n * kHidden + 255u) / 256u, 2048u)),
                           dim3(256), 0, st, io.hidden, nullptr, nullptr, n * kHidden);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    const unsigned blocks = (unsigned)std::min<uint64_t>(io.B / kPolRows + nseg, 512u);
    hipLaunchKernelGGL(policy_seq_eval_groups_kernel, dim3(blocks), dim3(256), kPolSeqEvalGroupLds, st, io, order,
                       segments, table, nseg);
    return hipGetLastError();
}

hipError_t launch_policy_seq_grad_groups(const PolSeqIO &io, const int32_t *order, const int32_t *segments,
                                         const PolSeqGroupSpec *specs, uint32_t nseg, const PolGroupWave *waves,
                                         const PolSeqGroupGrads *grads, uint32_t nwaves, float *ws, PolGroupEntry *table,
                                         PolUpload *uploads, float *slabs, uint64_t slab_stride, float *stash, float *hws,
                                         uint32_t wave_acc, hipStream_t st)
{
    static bool set = false;
    if (const hipError_t e =
            policy_seq_lds(reinterpret_cast<const void *>(policy_seq_grad_groups_kernel), kPolSeqGradGroupLds, set))
        return e;
    if (const hipError_t e = policy_seq_groups_prepare(specs, nseg, ws, table, uploads, false, st)) return e;
    for (uint32_t w = 0; w < nwaves; ++w) {
        if (wave_acc && io.L) {
            hipLaunchKernelGGL(policy_seq_grad_groups_kernel, dim3(wave_acc, waves[w].n), dim3(256), kPolSeqGradGroupLds,
                               st, io, order, segments, table, waves[w], slabs, slab_stride, stash, hws);
            if (const hipError_t e = hipGetLastError()) return e;
        }
        hipLaunchKernelGGL(policy_seq_grad_groups_reduce_kernel, dim3(16, kPolGateLayers, waves[w].n), dim3(256), 0, st,
                           segments, io.B, table, waves[w], grads[w], slabs, slab_stride, io.L ? wave_acc : 0u);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// counts[chunks][256] and the total (MBOTS_POLICY_SEQ_ORDER_WORKSPACE)
size_t policy_seq_order_workspace(uint64_t B)
{
    return ((size_t)((B + kPolOrderChunk - 1u) / kPolOrderChunk) * 256u + 64u) * 4u;
}

hipError_t launch_policy_seq_order(const int32_t *net_id, uint64_t B, uint32_t nkeys, int32_t *order, int32_t *segments,
                                   uint32_t *counts, hipStream_t st)
{
    const uint32_t nchunks = (uint32_t)((B + kPolOrderChunk - 1u) / kPolOrderChunk);
    if (nchunks) {
        hipLaunchKernelGGL(policy_seq_order_count_kernel, dim3(nchunks), dim3(256), 0, st, net_id, B, counts);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_seq_order_scan_kernel, dim3(1), dim3(256), 0, st, counts, nchunks, nkeys, segments);
    if (const hipError_t e = hipGetLastError()) return e;
    if (nchunks) {
        hipLaunchKernelGGL(policy_seq_order_scatter_kernel, dim3(nchunks), dim3(256), 0, st, net_id, B, counts, nchunks,
                           nkeys, order);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_policy_seq_eval(const PolSeqIO &io, const PolNet &net, hipStream_t st)
{
    if (io.B == 0 || io.L == 0) return hipSuccess;
    static bool set = false;
    if (const hipError_t e = policy_seq_lds(reinterpret_cast<const void *>(policy_seq_eval_kernel), kPolSeqEvalLds, set))
        return e;
    const uint64_t tiles = (io.B + kPolRows - 1u) / kPolRows;
    const unsigned blocks = (unsigned)std::min<uint64_t>(tiles, 512u);
    hipLaunchKernelGGL(policy_seq_eval_kernel, dim3(blocks), dim3(256), kPolSeqEvalLds, st, io, net);
    return hipGetLastError();
}

hipError_t launch_policy_seq_grad(const PolSeqIO &io, const PolNet &net, const PolNet &back, const PolGradSlabs &slabs,
                                  float *stash, float *hws, const PolGradOut &out, hipStream_t st)
{
    if (slabs.nacc) {
        static bool set = false;
        if (const hipError_t e =
                policy_seq_lds(reinterpret_cast<const void *>(policy_seq_grad_kernel), kPolSeqGradLds, set))
            return e;
        PolSeqGradDev G{back, slabs, stash, hws};
        hipLaunchKernelGGL(policy_seq_grad_kernel, dim3(slabs.nacc), dim3(256), kPolSeqGradLds, st, io, net, G);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_grad_reduce_kernel, dim3(16, out.n), dim3(256), 0, st, slabs, out);
    return hipGetLastError();
}

hipError_t launch_policy_act(const SimState &S, const ObsTable &t, const float *hidden_in, const PolNets &nets,
                             const PolGroups *groups, bool gated, uint32_t flags, const uint32_t *draw,
                             int32_t *action_out, float *logp_out, float *value_out, uint32_t out_rows,
                             uint32_t max_rows, hipStream_t st)
{
    // four kernels: one group or the groups' table, with or without the gate's code
    const void *fn = groups ? (gated ? reinterpret_cast<const void *>(policy_act_groups_kernel<true>)
                                     : reinterpret_cast<const void *>(policy_act_groups_kernel<false>))
                            : (gated ? reinterpret_cast<const void *>(policy_act_kernel<true>)
                                     : reinterpret_cast<const void *>(policy_act_kernel<false>));
    static bool lds_set[4] = {false, false, false, false};
    const int which = (groups ? 2 : 0) + (gated ? 1 : 0);
    if (!lds_set[which]) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(groups ? kPolGroupLds : kPolLds));
        if (e != hipSuccess) return e;
        lds_set[which] = true;
    }
    PolActArgs A{};
    A.totals = S.totals;
    A.scount = S.scount;
    A.row_base = S.row_base;
    A.sem = t.sem;
    A.depth = (S.flags & kFlagFixDepth) ? t.depth : reinterpret_cast<const uint8_t *>(t.sem);
    A.health = t.health;
    A.pos = t.pos;
    A.sur = t.sur;
    A.hidden_in = hidden_in;
    const bool write = !(flags & kActNoWrite);
    A.action = write ? t.action : nullptr;
    A.hidden_out = write ? t.hidden : nullptr;
    A.action_out = action_out;
    A.logp_out = logp_out;
    A.value_out = value_out;
    A.draw = draw;
    A.out_rows = out_rows;
    A.W = S.W;
    A.Wx = S.Wx;
    A.world_offset = S.world_offset;
    A.seed = S.seed;
    A.greedy = (flags & kActGreedy) ? 1u : 0u;
    // persistent: two blocks per compute unit at most (the LDS tile), never more
    // blocks than the table can hold tiles (8 segments, each with a ragged one)
    // (with groups: 4 G + 4 segments)
    const uint64_t tiles = (uint64_t)max_rows / kPolRows + (groups ? 4u * groups->G + 4u : 8u);
    const unsigned blocks = (unsigned)std::min<uint64_t>(tiles, 512u);
    if (groups && gated)
        hipLaunchKernelGGL(policy_act_groups_kernel<true>, dim3(blocks), dim3(256), kPolGroupLds, st, A, *groups);
    else if (groups)
        hipLaunchKernelGGL(policy_act_groups_kernel<false>, dim3(blocks), dim3(256), kPolGroupLds, st, A, *groups);
    else if (gated) hipLaunchKernelGGL(policy_act_kernel<true>, dim3(blocks), dim3(256), kPolLds, st, A, nets);
    else hipLaunchKernelGGL(policy_act_kernel<false>, dim3(blocks), dim3(256), kPolLds, st, A, nets);
    return hipGetLastError();
}

hipError_t launch_policy_segments(const SimState &S, const PolGroups &groups, int32_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(policy_segments_kernel, dim3(1), dim3(256), 0, st, S.totals, S.row_base, S.Wx, groups, out);
    return hipGetLastError();
}

hipError_t launch_policy_draw_next(uint32_t *draw, hipStream_t st)
{
    hipLaunchKernelGGL(policy_draw_next_kernel, dim3(1), dim3(1), 0, st, draw);
    return hipGetLastError();
}

hipError_t launch_policy_repack(const PolUploads &U, hipStream_t st)
{
    if (U.n == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_repack_kernel, dim3(32, U.n), dim3(256), 0, st, U);
    return hipGetLastError();
}

hipError_t launch_policy_activation(int act, const float *x, float *y, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(policy_activation_kernel, dim3(blocks), dim3(256), 0, st, act, x, y, n);
    return hipGetLastError();
}

// ---- the update on the device (mbots_policy.hpp; DESIGN.md "Device learner
// step") ----
// thread g: rows[g] += the group's four hi - lo (a segment with lo > hi or a
// negative bound counts as empty)
__global__ __launch_bounds__(64) void policy_group_rows_kernel(const int32_t *segments, uint32_t groups, int64_t *rows)
{
    for (uint32_t g = threadIdx.x; g < groups; g += 64u) {
        int64_t sum = 0;
        for (uint32_t s = 0; s < 4u; ++s) {
            const int32_t lo = segments[2u * (4u * g + s)], hi = segments[2u * (4u * g + s) + 1u];
            if (lo >= 0 && hi > lo) sum += (int64_t)hi - lo;
        }
        rows[g] += sum;
    }
}

// Block g is group g; its threads [256 s, 256 s + 256) are the accumulators of
// species s: thread a takes the rows a, a + 256, ... of the segment in
// ascending order, four in flight.  The order of the sums does not depend on
// the launch: the 256 accumulators in ascending index, the species ascending.
constexpr uint32_t kLossFlight = 4;
__global__ __launch_bounds__(1024) void policy_a2c_loss_kernel(PolLossIO A)
{
    __shared__ double s_acc[4u * kLossAcc];
    __shared__ double s_sum[4];
    const uint32_t g = blockIdx.x, s = uniform(threadIdx.x >> 8), a = threadIdx.x & (kLossAcc - 1u);
    uint32_t lo, len;
    pol_segment(A.segments, 4u * g + s, A.n, lo, len);
    lo = uniform(lo);
    len = uniform(len);
    const float scale = pol_loss_scale(A.rows[g]);
    const float *__restrict__ logp = A.logp, *__restrict__ value = A.value, *__restrict__ entropy = A.entropy;
    const float *__restrict__ adv = A.adv, *__restrict__ ret = A.ret;
    const int32_t *__restrict__ end = A.end;
    double acc = 0.0;
    for (uint32_t i0 = a; i0 < len; i0 += kLossFlight * kLossAcc) {
        float x[kLossFlight][5];
        int32_t e[kLossFlight];
#pragma unroll
        for (uint32_t k = 0; k < kLossFlight; ++k) {
            const uint32_t i = i0 + k * kLossAcc;
            if (i < len) {
                const uint64_t r = (uint64_t)lo + i;
                x[k][0] = logp[r], x[k][1] = value[r], x[k][2] = entropy[r], x[k][3] = adv[r], x[k][4] = ret[r];
                e[k] = end ? end[r] : 0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kLossFlight; ++k) {
            const uint32_t i = i0 + k * kLossAcc;
            if (i < len) {
                const uint64_t r = (uint64_t)lo + i;
                const float w = (e[k] == kTrajEndReset ? 0.0f : 1.0f) * scale;
                float gl, gv, ge;
                const float per_row = pol_loss_row(x[k][0], x[k][1], x[k][2], x[k][3], x[k][4], w, A.value_coef,
                                                   A.entropy_coef, gl, gv, ge);
                if (A.g_logp) A.g_logp[r] = gl;
                if (A.g_value) A.g_value[r] = gv;
                if (A.g_entropy) A.g_entropy[r] = ge;
                acc += (double)per_row;
            }
        }
    }
    if (A.loss == nullptr) return;
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (a == 0u) {
        double q = 0.0;
        for (uint32_t k = 0; k < kLossAcc; ++k) q += s_acc[s * kLossAcc + k];
        s_sum[s] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        double q = 0.0;
        for (uint32_t k = 0; k < 4u; ++k) q += s_sum[k];
        A.loss[g] += q;
    }
}

hipError_t launch_policy_group_rows(const int32_t *segments, uint32_t groups, int64_t *rows, hipStream_t st)
{
    hipLaunchKernelGGL(policy_group_rows_kernel, dim3(1), dim3(64), 0, st, segments, groups, rows);
    return hipGetLastError();
}

hipError_t launch_policy_a2c_loss(const PolLossIO &io, uint32_t groups, hipStream_t st)
{
    if (io.n && (io.g_logp || io.g_value || io.g_entropy)) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((io.n + 255u) / 256u, 2048u);
        hipLaunchKernelGGL(policy_zero_rows_kernel, dim3(blocks), dim3(256), 0, st, io.g_logp, io.g_value, io.g_entropy,
                           io.n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_a2c_loss_kernel, dim3(groups), dim3(1024), 0, st, io);
    return hipGetLastError();
}

// Adam over the launch's tensors: block b on one chunk of one tensor, found in
// the launch's prefix of chunk counts.  Every block reads its group's state as
// the previous step left it; policy_adam_advance_kernel follows in the stream.
__global__ __launch_bounds__(256) void policy_adam_kernel(AdamLaunch L, const AdamState *state, const int64_t *rows,
                                                          AdamCoef C)
{
    const uint32_t b = blockIdx.x;
    uint32_t lo = 0, hi = L.n - 1u;   // the last tensor whose first block is <= b
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (L.first[mid] <= b) lo = mid;
        else hi = mid - 1u;
    }
    const uint32_t i = uniform(lo);
    const uint32_t group = L.t[i].group;
    if (rows != nullptr && rows[group] == 0) return;
    const AdamState S = state[group];
    const float c1 = 1.0f - S.b1t * C.beta1, c2 = 1.0f - S.b2t * C.beta2;
    const uint64_t base = (uint64_t)(b - L.first[i]) * kAdamChunk;
    const uint32_t cnt = (uint32_t)min((uint64_t)kAdamChunk, L.t[i].n - base);
    float *__restrict__ p = L.t[i].param + base;
    const float *__restrict__ g = L.t[i].grad + base;
    float *__restrict__ m = L.t[i].m + base;
    float *__restrict__ v = L.t[i].v + base;
    const uint32_t t = threadIdx.x;
    const bool wide = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0u;
    if (wide) {
        static_assert(kAdamChunk == 4u * 256u, "policy_adam_kernel: one 16-byte access per thread and stream");
        if (4u * t + 4u <= cnt) {
            float4 P = reinterpret_cast<float4 *>(p)[t];
            const float4 Gr = reinterpret_cast<const float4 *>(g)[t];
            float4 M = reinterpret_cast<float4 *>(m)[t], V = reinterpret_cast<float4 *>(v)[t];
            pol_adam(P.x, Gr.x, M.x, V.x, C, c1, c2);
            pol_adam(P.y, Gr.y, M.y, V.y, C, c1, c2);
            pol_adam(P.z, Gr.z, M.z, V.z, C, c1, c2);
            pol_adam(P.w, Gr.w, M.w, V.w, C, c1, c2);
            reinterpret_cast<float4 *>(p)[t] = P;
            reinterpret_cast<float4 *>(m)[t] = M;
            reinterpret_cast<float4 *>(v)[t] = V;
        }
        const uint32_t k = (cnt & ~3u) + t;   // the scalar tail
        if (t < (cnt & 3u)) {
            float P = p[k], M = m[k], V = v[k];
            pol_adam(P, g[k], M, V, C, c1, c2);
            p[k] = P, m[k] = M, v[k] = V;
        }
        return;
    }
    for (uint32_t k = t; k < cnt; k += 256u) {
        float P = p[k], M = m[k], V = v[k];
        pol_adam(P, g[k], M, V, C, c1, c2);
        p[k] = P, m[k] = M, v[k] = V;
    }
}

__global__ __launch_bounds__(64) void policy_adam_advance_kernel(AdamState *state, const int64_t *rows, uint32_t groups,
                                                                 float beta1, float beta2)
{
    for (uint32_t g = threadIdx.x; g < groups; g += 64u) {
        if (rows != nullptr && rows[g] == 0) continue;
        AdamState S = state[g];
        S.t += 1u;
        S.b1t = S.b1t * beta1;
        S.b2t = S.b2t * beta2;
        state[g] = S;
    }
}

hipError_t launch_policy_adam(const AdamTensor *tensors, uint64_t count, AdamState *state, uint32_t groups,
                              const int64_t *rows, const AdamCoef &C, hipStream_t st)
{
    AdamLaunch L;
    L.n = 0;
    L.first[0] = 0;
    auto flush = [&]() -> hipError_t {
        if (L.n == 0 || L.first[L.n] == 0) return hipSuccess;
        hipLaunchKernelGGL(policy_adam_kernel, dim3(L.first[L.n]), dim3(256), 0, st, L, state, rows, C);
        L.n = 0;
        return hipGetLastError();
    };
    for (uint64_t i = 0; i < count; ++i) {
        if (tensors[i].n == 0) continue;
        L.t[L.n] = tensors[i];
        L.first[L.n + 1u] = L.first[L.n] + (uint32_t)((tensors[i].n + kAdamChunk - 1u) / kAdamChunk);
        if (++L.n == kAdamTensors)
            if (hipError_t e = flush()) return e;
    }
    if (hipError_t e = flush()) return e;
    hipLaunchKernelGGL(policy_adam_advance_kernel, dim3(1), dim3(64), 0, st, state, rows, groups, C.beta1, C.beta2);
    return hipGetLastError();
}

// ---- the sequence loss: the padded [L, B] batches of the recurrent learners ----
// column order[p]'s kept elements, its length read as at most `cap`: 0 where
// the entry names no column
__device__ __forceinline__ int32_t seq_kept(const PolSeqLossIO &A, int32_t col, int32_t cap)
{
    if ((uint64_t)(uint32_t)col >= A.B) return 0;
    return pol_seq_kept(min(A.len[col], cap), A.t0[col], A.end[col], A.last_table);
}

// blocks (g, 0 .. gridDim.y) share group g's positions; the counts are
// integers, so the order of the sum is free
__global__ __launch_bounds__(256) void policy_seq_group_rows_kernel(PolSeqLossIO A, int64_t *rows)
{
    __shared__ int64_t s_sum[256];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    int64_t sum = 0;
    for (uint32_t s = 0; s < 4u; ++s) {
        uint32_t lo, len;
        pol_segment(A.segments, 4u * g + s, A.B, lo, len);
        for (uint32_t i = blockIdx.y * 256u + t; i < len; i += gridDim.y * 256u) sum += seq_kept(A, A.order[lo + i], INT32_MAX);
    }
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t h = 128u; h > 0u; h >>= 1) {
        if (t < h) s_sum[t] += s_sum[t + h];
        __syncthreads();
    }
    if (t == 0u && s_sum[0] != 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(rows + g), (unsigned long long)s_sum[0]);
}

// Block g is group g, threads [256 s, 256 s + 256) the accumulators of species
// s, as policy_a2c_loss_kernel: thread a takes the columns at positions a,
// a + 256, ... of the segment in ascending order and each column's kept steps
// in ascending k, so the order of the sums is a property of the indices alone.
// The metadata and the first kSeqSteps steps of kSeqFlight columns are loaded
// before the first is consumed; a longer column reloads its own registers.
constexpr uint32_t kSeqFlight = 4, kSeqSteps = 4;
__global__ __launch_bounds__(1024) void policy_seq_a2c_loss_kernel(PolSeqLossIO A)
{
    __shared__ double s_acc[4u * kLossAcc];
    __shared__ double s_sum[4];
    const uint32_t g = blockIdx.x, s = uniform(threadIdx.x >> 8), a = threadIdx.x & (kLossAcc - 1u);
    const int64_t rows = A.rows[g];
    if (rows == 0) return;   // the whole block: the fill's +0 stay, the loss is not touched
    uint32_t lo, len;
    pol_segment(A.segments, 4u * g + s, A.B, lo, len);
    lo = uniform(lo);
    len = uniform(len);
    const float w = pol_loss_scale(rows);
    const float *__restrict__ logp = A.logp, *__restrict__ value = A.value, *__restrict__ entropy = A.entropy;
    const float *__restrict__ adv = A.adv, *__restrict__ ret = A.ret;
    const uint64_t B = A.B;
    double acc = 0.0;
    for (uint32_t i0 = a; i0 < len; i0 += kSeqFlight * kLossAcc) {
        int32_t col[kSeqFlight], nk[kSeqFlight];
        float x[kSeqFlight][kSeqSteps][5];
#pragma unroll
        for (uint32_t c = 0; c < kSeqFlight; ++c) {
            const uint32_t i = i0 + c * kLossAcc;
            col[c] = i < len ? A.order[lo + i] : -1;
        }
#pragma unroll
        for (uint32_t c = 0; c < kSeqFlight; ++c) nk[c] = seq_kept(A, col[c], (int32_t)A.L);
        auto load = [&](uint32_t c, int32_t k0) {
#pragma unroll
            for (uint32_t j = 0; j < kSeqSteps; ++j)
                if (k0 + (int32_t)j < nk[c]) {
                    const uint64_t r = (uint64_t)(k0 + (int32_t)j) * B + (uint32_t)col[c];
                    x[c][j][0] = logp[r], x[c][j][1] = value[r], x[c][j][2] = entropy[r], x[c][j][3] = adv[r];
                    x[c][j][4] = ret[r];
                }
        };
#pragma unroll
        for (uint32_t c = 0; c < kSeqFlight; ++c) load(c, 0);
#pragma unroll
        for (uint32_t c = 0; c < kSeqFlight; ++c) {
            for (int32_t k0 = 0; k0 < nk[c]; k0 += (int32_t)kSeqSteps) {
                if (k0) load(c, k0);
#pragma unroll
                for (uint32_t j = 0; j < kSeqSteps; ++j)
                    if (k0 + (int32_t)j < nk[c]) {
                        const uint64_t r = (uint64_t)(k0 + (int32_t)j) * B + (uint32_t)col[c];
                        float gl, gv, ge;
                        const float per_row = pol_loss_row(x[c][j][0], x[c][j][1], x[c][j][2], x[c][j][3], x[c][j][4],
                                                           w, A.value_coef, A.entropy_coef, gl, gv, ge);
                        if (A.g_logp) A.g_logp[r] = gl;
                        if (A.g_value) A.g_value[r] = gv;
                        if (A.g_entropy) A.g_entropy[r] = ge;
                        acc += (double)per_row;
                    }
            }
        }
    }
    if (A.loss == nullptr) return;
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (a == 0u) {
        double q = 0.0;
        for (uint32_t k = 0; k < kLossAcc; ++k) q += s_acc[s * kLossAcc + k];
        s_sum[s] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        double q = 0.0;
        for (uint32_t k = 0; k < 4u; ++k) q += s_sum[k];
        A.loss[g] += q;
    }
}

hipError_t launch_policy_seq_group_rows(const PolSeqLossIO &io, uint32_t groups, int64_t *rows, hipStream_t st)
{
    if (io.B == 0) return hipSuccess;
    const unsigned per = (unsigned)std::min<uint64_t>((io.B + 1023u) / 1024u, 32u);
    hipLaunchKernelGGL(policy_seq_group_rows_kernel, dim3(groups, per), dim3(256), 0, st, io, rows);
    return hipGetLastError();
}

hipError_t launch_policy_seq_a2c_loss(const PolSeqLossIO &io, uint32_t groups, hipStream_t st)
{
    const uint64_t n = (uint64_t)io.L * io.B;
    if (n && (io.g_logp || io.g_value || io.g_entropy)) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255u) / 256u, 2048u);
        hipLaunchKernelGGL(policy_zero_rows_kernel, dim3(blocks), dim3(256), 0, st, io.g_logp, io.g_value, io.g_entropy, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_seq_a2c_loss_kernel, dim3(groups), dim3(1024), 0, st, io);
    return hipGetLastError();
}

// ---- mbots_policy_adam_clip ----
// block b's tensor of the launch: the last whose first block is <= b
__device__ __forceinline__ uint32_t adam_tensor_of(const uint32_t *first, uint32_t n, uint32_t b)
{
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (first[mid] <= b) lo = mid;
        else hi = mid - 1u;
    }
    return uniform(lo);
}

// q[chunk0 + b]: the squared norm of block b's chunk of the gradient, thread t
// the accumulator of elements 4t .. 4t + 3 -- from one 16-byte load or from
// four 4-byte loads, the same values either way -- and the tree over the 256
__global__ __launch_bounds__(256) void policy_adam_sq_kernel(AdamLaunch L, uint32_t chunk0, double *q)
{
    __shared__ double s_a[256];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint32_t i = adam_tensor_of(L.first, L.n, b);
    const uint64_t base = (uint64_t)(b - L.first[i]) * kAdamChunk;
    const uint32_t cnt = (uint32_t)min((uint64_t)kAdamChunk, L.t[i].n - base);
    const float *__restrict__ g = L.t[i].grad + base;
    static_assert(kAdamChunk == 4u * 256u, "policy_adam_sq_kernel: four elements per thread");
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (((uintptr_t)g & 15u) == 0u && 4u * t + 4u <= cnt) {
        const float4 G = reinterpret_cast<const float4 *>(g)[t];
        x[0] = G.x, x[1] = G.y, x[2] = G.z, x[3] = G.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (4u * t + k < cnt) x[k] = g[4u * t + k];
    }
    s_a[t] = pol_sq4(x[0], x[1], x[2], x[3]);
    __syncthreads();
    for (uint32_t h = 128u; h > 0u; h >>= 1) {
        if (t < h) s_a[t] = s_a[t] + s_a[t + h];
        __syncthreads();
    }
    if (t == 0u) q[chunk0 + b] = s_a[0];
}

// one block: thread i the ascending sum of tensor i's chunk partials, then
// thread g group g's tensors of this launch in descriptor order, onto what
// the earlier launches of the call left (`first`: onto +0)
__global__ __launch_bounds__(64) void policy_adam_fold_kernel(AdamFold F, AdamClipWs W, uint32_t groups, int first)
{
    __shared__ double s_t[kAdamTensors];
    const uint32_t t = threadIdx.x;
    if (t < F.n) {
        double sum = 0.0;
        for (uint32_t c = F.first[t]; c < F.first[t + 1u]; ++c) sum += W.q[c];
        s_t[t] = sum;
        W.tsum[F.slot[t]] = sum;
    }
    __syncthreads();
    static_assert(kPolMaxGroups <= 64u, "policy_adam_fold_kernel: one thread per group");
    if (t < groups) {
        double n2 = first ? 0.0 : W.normsq[t];
        for (uint32_t i = 0; i < F.n; ++i)
            if (F.group[i] == t) n2 += s_t[i];
        W.normsq[t] = n2;
    }
}

// thread g: group g's norm, clip factor and whether it takes the step
__global__ __launch_bounds__(64) void policy_adam_finish_kernel(AdamClipWs W, const int64_t *rows, uint32_t groups,
                                                                AdamClipCoef K, float *grad_norm)
{
    const uint32_t g = threadIdx.x;
    if (g >= groups) return;
    float nrm, coef;
    const bool finite = pol_clip_coef(W.normsq[g], K, nrm, coef);
    W.coef[g] = coef;
    W.live[g] = finite && (rows == nullptr || rows[g] != 0) ? 1u : 0u;
    if (grad_norm) grad_norm[g] = nrm;
}

// policy_adam_kernel on the clipped gradient and the decayed parameter, for
// the groups the finish kernel left live
__global__ __launch_bounds__(256) void policy_adam_clip_kernel(AdamLaunch L, const AdamState *state, AdamClipWs W,
                                                               AdamCoef C, AdamClipCoef K)
{
    const uint32_t b = blockIdx.x;
    const uint32_t i = adam_tensor_of(L.first, L.n, b);
    const uint32_t group = L.t[i].group;
    if (W.live[group] == 0u) return;
    const float coef = W.coef[group];
    const AdamState S = state[group];
    const float c1 = 1.0f - S.b1t * C.beta1, c2 = 1.0f - S.b2t * C.beta2;
    const uint64_t base = (uint64_t)(b - L.first[i]) * kAdamChunk;
    const uint32_t cnt = (uint32_t)min((uint64_t)kAdamChunk, L.t[i].n - base);
    float *__restrict__ p = L.t[i].param + base;
    const float *__restrict__ g = L.t[i].grad + base;
    float *__restrict__ m = L.t[i].m + base;
    float *__restrict__ v = L.t[i].v + base;
    const uint32_t t = threadIdx.x;
    const bool wide = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0u;
    if (wide) {
        if (4u * t + 4u <= cnt) {
            float4 P = reinterpret_cast<float4 *>(p)[t];
            const float4 Gr = reinterpret_cast<const float4 *>(g)[t];
            float4 M = reinterpret_cast<float4 *>(m)[t], V = reinterpret_cast<float4 *>(v)[t];
            pol_adam_clip(P.x, Gr.x, M.x, V.x, C, K, coef, c1, c2);
            pol_adam_clip(P.y, Gr.y, M.y, V.y, C, K, coef, c1, c2);
            pol_adam_clip(P.z, Gr.z, M.z, V.z, C, K, coef, c1, c2);
            pol_adam_clip(P.w, Gr.w, M.w, V.w, C, K, coef, c1, c2);
            reinterpret_cast<float4 *>(p)[t] = P;
            reinterpret_cast<float4 *>(m)[t] = M;
            reinterpret_cast<float4 *>(v)[t] = V;
        }
        const uint32_t k = (cnt & ~3u) + t;   // the scalar tail
        if (t < (cnt & 3u)) {
            float P = p[k], M = m[k], V = v[k];
            pol_adam_clip(P, g[k], M, V, C, K, coef, c1, c2);
            p[k] = P, m[k] = M, v[k] = V;
        }
        return;
    }
    for (uint32_t k = t; k < cnt; k += 256u) {
        float P = p[k], M = m[k], V = v[k];
        pol_adam_clip(P, g[k], M, V, C, K, coef, c1, c2);
        p[k] = P, m[k] = M, v[k] = V;
    }
}

__global__ __launch_bounds__(64) void policy_adam_clip_advance_kernel(AdamState *state, const uint32_t *live,
                                                                      uint32_t groups, float beta1, float beta2)
{
    for (uint32_t g = threadIdx.x; g < groups; g += 64u) {
        if (live[g] == 0u) continue;
        AdamState S = state[g];
        S.t += 1u;
        S.b1t = S.b1t * beta1;
        S.b2t = S.b2t * beta2;
        state[g] = S;
    }
}

void policy_adam_clip_counts(const AdamTensor *tensors, uint64_t count, uint64_t &chunks, uint64_t &present)
{
    chunks = present = 0;
    for (uint64_t i = 0; i < count; ++i)
        if (tensors[i].n) chunks += (tensors[i].n + kAdamChunk - 1u) / kAdamChunk, ++present;
}

hipError_t launch_policy_adam_clip(const AdamTensor *tensors, uint64_t count, AdamState *state, uint32_t groups,
                                   const int64_t *rows, const AdamCoef &C, const AdamClipCoef &K, float *grad_norm,
                                   void *workspace, hipStream_t st)
{
    uint64_t chunks, present;
    policy_adam_clip_counts(tensors, count, chunks, present);
    const AdamClipWs W = pol_adam_clip_ws(workspace, chunks, present, groups);
    // the launches of 64 tensors, as launch_policy_adam cuts them
    AdamLaunch L;
    AdamFold F;
    uint32_t chunk0 = 0, slot = 0;
    int first = 1;
    auto each_launch = [&](auto &&fn) -> hipError_t {
        L.n = 0, L.first[0] = 0;
        for (uint64_t i = 0; i <= count; ++i) {
            if (i < count && tensors[i].n) {
                L.t[L.n] = tensors[i];
                L.first[L.n + 1u] = L.first[L.n] + (uint32_t)((tensors[i].n + kAdamChunk - 1u) / kAdamChunk);
                ++L.n;
            }
            if (L.n == kAdamTensors || (i == count && L.n)) {
                if (hipError_t e = fn()) return e;
                L.n = 0;
            }
        }
        return hipSuccess;
    };
    if (hipError_t e = each_launch([&]() -> hipError_t {
            hipLaunchKernelGGL(policy_adam_sq_kernel, dim3(L.first[L.n]), dim3(256), 0, st, L, chunk0, W.q);
            if (hipError_t e = hipGetLastError()) return e;
            F.n = L.n;
            for (uint32_t i = 0; i < L.n; ++i) {
                F.first[i] = chunk0 + L.first[i];
                F.slot[i] = slot++;
                F.group[i] = L.t[i].group;
            }
            F.first[L.n] = chunk0 + L.first[L.n];
            chunk0 += L.first[L.n];
            hipLaunchKernelGGL(policy_adam_fold_kernel, dim3(1), dim3(64), 0, st, F, W, groups, first);
            first = 0;
            return hipGetLastError();
        }))
        return e;
    if (first) {   // no gradient at all: every norm is +0
        F.n = 0;
        hipLaunchKernelGGL(policy_adam_fold_kernel, dim3(1), dim3(64), 0, st, F, W, groups, 1);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(policy_adam_finish_kernel, dim3(1), dim3(64), 0, st, W, rows, groups, K, grad_norm);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = each_launch([&]() -> hipError_t {
            hipLaunchKernelGGL(policy_adam_clip_kernel, dim3(L.first[L.n]), dim3(256), 0, st, L, state, W, C, K);
            return hipGetLastError();
        }))
        return e;
    hipLaunchKernelGGL(policy_adam_clip_advance_kernel, dim3(1), dim3(64), 0, st, state, W.live, groups, C.beta1, C.beta2);
    return hipGetLastError();
}

// ---- PPO on the device (mbots_policy.hpp "PPO on the device") ----
// Block (c, s, g) is chunk c of species s of group g, its 256 threads the
// chunk's accumulators: thread a takes the elements a, a + 256, ... of the
// chunk in ascending order.  A block whose chunk lies past the segment's end
// exits at once, so the grid is sized from n and the group count alone and the
// order of the sums -- accumulators, chunks, species, each ascending -- is a
// property of the indices.
constexpr uint32_t kPpoFlight = 4;

// the block's chunk of segment (g, s): first element and element count; false: past the end
__device__ __forceinline__ bool ppo_chunk(const int32_t *segments, uint64_t n, uint32_t chunk, uint32_t &lo,
                                          uint32_t &cnt)
{
    uint32_t len;
    pol_segment(segments, 4u * blockIdx.z + blockIdx.y, n, lo, len);
    const uint64_t first = (uint64_t)blockIdx.x * chunk;
    if (first >= len) return false;
    lo = uniform(lo + (uint32_t)first);
    cnt = uniform(min(chunk, len - (uint32_t)first));
    return true;
}

// the 256 accumulators of kSlots sums meet in LDS; thread k < kSlots adds slot
// k's in ascending index and leaves the chunk's partial
template <uint32_t kSlots>
__device__ __forceinline__ void ppo_chunk_fold(double (*s_acc)[kLossAcc], const double *acc, double *part,
                                               uint32_t chunks)
{
    const uint32_t a = threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kSlots; ++k) s_acc[k][a] = acc[k];
    __syncthreads();
    if (a < kSlots) {
        double q = 0.0;
        for (uint32_t j = 0; j < kLossAcc; ++j) q += s_acc[a][j];
        part[(((size_t)(4u * blockIdx.z + blockIdx.y)) * chunks + blockIdx.x) * kSlots + a] = q;
    }
}

__global__ __launch_bounds__(256) void policy_adv_moments_kernel(PolPpoIO A)
{
    __shared__ double s_acc[kPpoMoments][kLossAcc];
    uint32_t lo, cnt;
    if (!ppo_chunk(A.segments, A.n, kPpoChunk, lo, cnt)) return;
    const float *__restrict__ adv = A.adv;
    const int32_t *__restrict__ end = A.end;
    double acc[kPpoMoments] = {0.0, 0.0, 0.0};
    for (uint32_t i0 = threadIdx.x; i0 < cnt; i0 += kPpoFlight * kLossAcc) {
        float x[kPpoFlight];
        int32_t e[kPpoFlight];
#pragma unroll
        for (uint32_t k = 0; k < kPpoFlight; ++k) {
            const uint32_t i = i0 + k * kLossAcc;
            if (i < cnt) {
                const uint64_t r = (uint64_t)lo + i;
                x[k] = adv[r];
                e[k] = end ? end[r] : 0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kPpoFlight; ++k)
            if (i0 + k * kLossAcc < cnt && e[k] != kTrajEndReset) pol_ppo_moment_add(acc, x[k]);
    }
    ppo_chunk_fold<kPpoMoments>(s_acc, acc, A.part, A.chunks);
}

__global__ __launch_bounds__(256) void policy_ppo_loss_kernel(PolPpoIO A)
{
    __shared__ double s_acc[kPpoStats][kLossAcc];
    uint32_t lo, cnt;
    if (!ppo_chunk(A.segments, A.n, kPpoChunk, lo, cnt)) return;
    const uint32_t g = blockIdx.z;
    const float scale = pol_loss_scale(A.rows[g]);
    const bool normalise = A.moments != nullptr;
    const PpoNorm N = pol_ppo_norm(normalise ? A.moments + (size_t)kPpoMoments * g : nullptr);
    const float *__restrict__ logp = A.logp, *__restrict__ value = A.value, *__restrict__ entropy = A.entropy;
    const float *__restrict__ old_logp = A.old_logp, *__restrict__ old_value = A.old_value;
    const float *__restrict__ adv = A.adv, *__restrict__ ret = A.ret;
    const int32_t *__restrict__ end = A.end;
    double acc[kPpoStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i0 = threadIdx.x; i0 < cnt; i0 += kPpoFlight * kLossAcc) {
        float x[kPpoFlight][7];
        int32_t e[kPpoFlight];
#pragma unroll
        for (uint32_t k = 0; k < kPpoFlight; ++k) {
            const uint32_t i = i0 + k * kLossAcc;
            if (i < cnt) {
                const uint64_t r = (uint64_t)lo + i;
                x[k][0] = logp[r], x[k][1] = value[r], x[k][2] = entropy[r], x[k][3] = old_logp[r];
                x[k][4] = A.C.vclip ? old_value[r] : 0.0f;
                x[k][5] = adv[r], x[k][6] = ret[r];
                e[k] = end ? end[r] : 0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kPpoFlight; ++k) {
            const uint32_t i = i0 + k * kLossAcc;
            if (i < cnt) {
                const uint64_t r = (uint64_t)lo + i;
                const float w = (e[k] == kTrajEndReset ? 0.0f : 1.0f) * scale;
                float gl, gv, ge, st[kPpoStats];
                pol_ppo_row(x[k][0], x[k][1], x[k][2], x[k][3], x[k][4], x[k][5], x[k][6], w, normalise, N, A.C, gl, gv,
                            ge, st);
                if (A.g_logp) A.g_logp[r] = gl;
                if (A.g_value) A.g_value[r] = gv;
                if (A.g_entropy) A.g_entropy[r] = ge;
#pragma unroll
                for (uint32_t j = 0; j < kPpoStats; ++j) acc[j] += (double)st[j];
            }
        }
    }
    if (A.out == nullptr) return;
    ppo_chunk_fold<kPpoStats>(s_acc, acc, A.part, A.chunks);
}

// Block g, thread (s, k) of its first 4 * slots: slot k of segment (g, s)'s
// chunk partials in ascending chunk; then thread k: the four species ascending,
// and out[g][k] += that.  skip (may be null): a group with skip[g] == 0 left
// no partials and is passed over.
__global__ __launch_bounds__(64) void policy_ppo_fold_kernel(const int32_t *segments, uint64_t n, uint32_t chunk,
                                                             uint32_t chunks, uint32_t slots, const double *part,
                                                             const int64_t *skip, double *out)
{
    __shared__ double s_sum[4][kPpoStats];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    if (skip && skip[g] == 0) return;
    if (t < 4u * slots) {
        const uint32_t s = t / slots, k = t - s * slots;
        uint32_t lo, len;
        pol_segment(segments, 4u * g + s, n, lo, len);
        const uint32_t nch = (uint32_t)(((uint64_t)len + chunk - 1u) / chunk);
        const double *p = part + ((size_t)(4u * g + s) * chunks) * slots + k;
        double q = 0.0;
        for (uint32_t c = 0; c < nch; ++c) q += p[(size_t)c * slots];
        s_sum[s][k] = q;
    }
    __syncthreads();
    if (t < slots) {
        double q = 0.0;
        for (uint32_t s = 0; s < 4u; ++s) q += s_sum[s][t];
        out[(size_t)g * slots + t] += q;
    }
}
static_assert(4u * kPpoStats <= 64u, "policy_ppo_fold_kernel: one thread per (species, slot)");

// column col's kept elements, its length read as at most L: 0 where the entry
// names no column
__device__ __forceinline__ int32_t ppo_seq_kept(const PolSeqPpoIO &A, int32_t col)
{
    if ((uint64_t)(uint32_t)col >= A.B) return 0;
    return pol_seq_kept(min(A.len[col], (int32_t)A.L), A.t0[col], A.end[col], A.last_table);
}

// the sequence twins: an element is a column position of the segment, its kept
// steps added in ascending k
__global__ __launch_bounds__(256) void policy_seq_adv_moments_kernel(PolSeqPpoIO A)
{
    __shared__ double s_acc[kPpoMoments][kLossAcc];
    uint32_t lo, cnt;
    if (!ppo_chunk(A.segments, A.B, kPpoSeqChunk, lo, cnt)) return;
    const float *__restrict__ adv = A.adv;
    const uint64_t B = A.B;
    double acc[kPpoMoments] = {0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < cnt; i += kLossAcc) {
        const int32_t col = A.order[lo + i], nk = ppo_seq_kept(A, col);
        for (int32_t k0 = 0; k0 < nk; k0 += (int32_t)kSeqSteps) {
            float x[kSeqSteps];
#pragma unroll
            for (uint32_t j = 0; j < kSeqSteps; ++j)
                if (k0 + (int32_t)j < nk) x[j] = adv[(uint64_t)(k0 + (int32_t)j) * B + (uint32_t)col];
#pragma unroll
            for (uint32_t j = 0; j < kSeqSteps; ++j)
                if (k0 + (int32_t)j < nk) pol_ppo_moment_add(acc, x[j]);
        }
    }
    ppo_chunk_fold<kPpoMoments>(s_acc, acc, A.part, A.chunks);
}

__global__ __launch_bounds__(256) void policy_seq_ppo_loss_kernel(PolSeqPpoIO A)
{
    __shared__ double s_acc[kPpoStats][kLossAcc];
    const uint32_t g = blockIdx.z;
    const int64_t rows = A.rows[g];
    if (rows == 0) return;   // the whole block: the fill's +0 stay, the statistics are not touched
    uint32_t lo, cnt;
    if (!ppo_chunk(A.segments, A.B, kPpoSeqChunk, lo, cnt)) return;
    const float w = pol_loss_scale(rows);
    const bool normalise = A.moments != nullptr;
    const PpoNorm N = pol_ppo_norm(normalise ? A.moments + (size_t)kPpoMoments * g : nullptr);
    const float *__restrict__ logp = A.logp, *__restrict__ value = A.value, *__restrict__ entropy = A.entropy;
    const float *__restrict__ old_logp = A.old_logp, *__restrict__ old_value = A.old_value;
    const float *__restrict__ adv = A.adv, *__restrict__ ret = A.ret;
    const uint64_t B = A.B;
    double acc[kPpoStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < cnt; i += kLossAcc) {
        const int32_t col = A.order[lo + i], nk = ppo_seq_kept(A, col);
        for (int32_t k0 = 0; k0 < nk; k0 += (int32_t)kSeqSteps) {
            float x[kSeqSteps][7];
#pragma unroll
            for (uint32_t j = 0; j < kSeqSteps; ++j)
                if (k0 + (int32_t)j < nk) {
                    const uint64_t r = (uint64_t)(k0 + (int32_t)j) * B + (uint32_t)col;
                    x[j][0] = logp[r], x[j][1] = value[r], x[j][2] = entropy[r], x[j][3] = old_logp[r];
                    x[j][4] = A.C.vclip ? old_value[r] : 0.0f;
                    x[j][5] = adv[r], x[j][6] = ret[r];
                }
#pragma unroll
            for (uint32_t j = 0; j < kSeqSteps; ++j)
                if (k0 + (int32_t)j < nk) {
                    const uint64_t r = (uint64_t)(k0 + (int32_t)j) * B + (uint32_t)col;
                    float gl, gv, ge, st[kPpoStats];
                    pol_ppo_row(x[j][0], x[j][1], x[j][2], x[j][3], x[j][4], x[j][5], x[j][6], w, normalise, N, A.C, gl,
                                gv, ge, st);
                    if (A.g_logp) A.g_logp[r] = gl;
                    if (A.g_value) A.g_value[r] = gv;
                    if (A.g_entropy) A.g_entropy[r] = ge;
#pragma unroll
                    for (uint32_t q = 0; q < kPpoStats; ++q) acc[q] += (double)st[q];
                }
        }
    }
    if (A.out == nullptr) return;
    ppo_chunk_fold<kPpoStats>(s_acc, acc, A.part, A.chunks);
}

// thread g: the gate of group g from its KL sum, stats[g][4]
__global__ __launch_bounds__(64) void policy_ppo_gate_kernel(const double *stats, const int64_t *rows, double target_kl,
                                                             int64_t *gate, uint32_t groups)
{
    static_assert(kPolMaxGroups <= 64u, "policy_ppo_gate_kernel: one thread per group");
    const uint32_t g = threadIdx.x;
    if (g < groups) gate[g] = pol_ppo_gate(gate[g], rows[g], stats[(size_t)kPpoStats * g + 4u], target_kl);
}

namespace {
hipError_t ppo_zero(float *a, float *b, float *c, uint64_t n, hipStream_t st)
{
    if (n == 0 || !(a || b || c)) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(policy_zero_rows_kernel, dim3(blocks), dim3(256), 0, st, a, b, c, n);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_policy_adv_moments(const PolPpoIO &io, uint32_t groups, hipStream_t st)
{
    if (io.chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_adv_moments_kernel, dim3(io.chunks, 4, groups), dim3(256), 0, st, io);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(policy_ppo_fold_kernel, dim3(groups), dim3(64), 0, st, io.segments, io.n, kPpoChunk, io.chunks,
                       kPpoMoments, io.part, (const int64_t *)nullptr, io.out);
    return hipGetLastError();
}

hipError_t launch_policy_ppo_loss(const PolPpoIO &io, uint32_t groups, hipStream_t st)
{
    if (hipError_t e = ppo_zero(io.g_logp, io.g_value, io.g_entropy, io.n, st)) return e;
    if (io.chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_ppo_loss_kernel, dim3(io.chunks, 4, groups), dim3(256), 0, st, io);
    if (hipError_t e = hipGetLastError()) return e;
    if (io.out == nullptr) return hipSuccess;
    hipLaunchKernelGGL(policy_ppo_fold_kernel, dim3(groups), dim3(64), 0, st, io.segments, io.n, kPpoChunk, io.chunks,
                       kPpoStats, io.part, (const int64_t *)nullptr, io.out);
    return hipGetLastError();
}

hipError_t launch_policy_seq_adv_moments(const PolSeqPpoIO &io, uint32_t groups, hipStream_t st)
{
    if (io.chunks == 0 || io.L == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_seq_adv_moments_kernel, dim3(io.chunks, 4, groups), dim3(256), 0, st, io);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(policy_ppo_fold_kernel, dim3(groups), dim3(64), 0, st, io.segments, io.B, kPpoSeqChunk, io.chunks,
                       kPpoMoments, io.part, (const int64_t *)nullptr, io.out);
    return hipGetLastError();
}

hipError_t launch_policy_seq_ppo_loss(const PolSeqPpoIO &io, uint32_t groups, hipStream_t st)
{
    if (hipError_t e = ppo_zero(io.g_logp, io.g_value, io.g_entropy, (uint64_t)io.L * io.B, st)) return e;
    if (io.chunks == 0 || io.L == 0) return hipSuccess;
    hipLaunchKernelGGL(policy_seq_ppo_loss_kernel, dim3(io.chunks, 4, groups), dim3(256), 0, st, io);
    if (hipError_t e = hipGetLastError()) return e;
    if (io.out == nullptr) return hipSuccess;
    hipLaunchKernelGGL(policy_ppo_fold_kernel, dim3(groups), dim3(64), 0, st, io.segments, io.B, kPpoSeqChunk, io.chunks,
                       kPpoStats, io.part, io.rows, io.out);
    return hipGetLastError();
}

hipError_t launch_policy_ppo_gate(const double *stats, const int64_t *rows, double target_kl, int64_t *gate,
                                  uint32_t groups, hipStream_t st)
{
    hipLaunchKernelGGL(policy_ppo_gate_kernel, dim3(1), dim3(64), 0, st, stats, rows, target_kl, gate, groups);
    return hipGetLastError();
}

}  // namespace mbots
