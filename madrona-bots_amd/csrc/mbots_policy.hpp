// mbots_policy.hpp -- the device actor (include/mbots.h "Acting on the
// device"; DESIGN.md "Device actor"): the arithmetic of the per-species policy
// nets, their activations and the action sampling, shared by the HIP kernel
// (mbots_kernels.hip) and the CPU mode's loops (mbots_cpu.cpp) so that both
// give the same bits.
//
// Everything here is built from + - * /, fmaf, comparisons and integer
// operations on the bits only -- no libm / ocml transcendental -- so the host
// build (-ffp-contract=off) and the device round every step alike.
#pragma once

#include "mbots_device.hpp"

#include <cmath>
#include <cstdint>

namespace mbots {

constexpr int kPolObs = 69;            // construct_obs(prev = False) floats of a row
constexpr int kPolActions = 6;
constexpr int kPolMaxH = 128;          // trunk width: a multiple of 16 in [16, 128]
constexpr int kPolMaxTrunk = 4;
constexpr int kPolLayers = kPolMaxTrunk + 6;   // trunk, actor 2, critic 2, memory, gate
constexpr uint32_t kPolMemoryIn = 1u;  // MBOTS_POLICY_MEMORY_IN
constexpr uint32_t kPolGate = 2u;      // MBOTS_POLICY_GATE
constexpr uint32_t kActGreedy = 1u, kActNoWrite = 2u;   // MBOTS_ACT_*
// activation codes (mbots_policy_layer.act; 6, 7 and 8 only through
// mbots_policy_activation)
constexpr int kActIdentity = 0, kActRelu = 1, kActLeaky = 2, kActTanh = 3, kActElu = 4, kActLogSigmoid = 5,
              kActExp = 6, kActLog = 7, kActSigmoid = 8;

// input width rounded up to the k-step of the matrix instruction
MB_HD uint32_t pol_kp(uint32_t in) { return (in + 3u) & ~3u; }

MB_HD float pol_fma(float a, float b, float c)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fmaf_rn(a, b, c);
#else
    return std::fmaf(a, b, c);
#endif
}

// ln 2 in two parts: n * kLn2Hi is exact for |n| < 512
constexpr float kLn2Hi = 0.693145751953125f, kLn2Lo = 1.42860654e-6f, kLog2e = 1.44269504f;

MB_HD float pol_pow2(int32_t n) { return u2f((uint32_t)(n + 127) << 23); }   // n in [-126, 127]

// range reduction of exp: y = n ln 2 + r, |r| <= ln 2 / 2 (+ a rounding)
MB_HD float pol_reduce(float y, int32_t &n)
{
    const float t = y * kLog2e;
    n = (int32_t)(t + (t < 0.0f ? -0.5f : 0.5f));
    const float nf = (float)n;
    return pol_fma(nf, -kLn2Lo, pol_fma(nf, -kLn2Hi, y));
}
// exp(r) - 1 on the reduced range: r + r^2 (1/2 + r/6 + ... + r^6/8!)
MB_HD float pol_expm1_r(float r)
{
    float q = 1.0f / 40320.0f;
    q = pol_fma(q, r, 1.0f / 5040.0f);
    q = pol_fma(q, r, 1.0f / 720.0f);
    q = pol_fma(q, r, 1.0f / 120.0f);
    q = pol_fma(q, r, 1.0f / 24.0f);
    q = pol_fma(q, r, 1.0f / 6.0f);
    q = pol_fma(q, r, 0.5f);
    return pol_fma(r * r, q, r);
}

// exp(x): 2^n (1 + expm1(r)), the scale applied in two exact-or-once-rounded
// halves so that results down to the subnormals round once
MB_HD float pol_exp(float x)
{
    if (!(x == x)) return x;
    if (x > 88.72284f) return u2f(0x7F800000u);
    if (x < -104.0f) return 0.0f;
    int32_t n;
    const float r = pol_reduce(x, n);
    const float p = pol_expm1_r(r) + 1.0f;
    const int32_t n1 = n >> 1, n2 = n - n1;
    return (p * pol_pow2(n1)) * pol_pow2(n2);
}

// exp(y) - 1 for y in [-18, 19]: near 0 (n == 0) the series itself, else
// (2^n - 1) + 2^n expm1(r) in one fmaf (2^n - 1 is exact up to n = 24)
MB_HD float pol_expm1(float y)
{
    int32_t n;
    const float r = pol_reduce(y, n);
    const float e = pol_expm1_r(r);
    if (n == 0) return e;
    const float s = pol_pow2(n);
    return pol_fma(s, e, s - 1.0f);
}

// log(1 + f) for f in [sqrt(1/2) - 1, sqrt(2) - 1]: s = f / (2 + f),
// log(1 + f) = 2 atanh(s) = f - s (f - 2 P), P = s^2/3 + s^4/5 + ... + s^12/13
MB_HD float pol_log1p_f(float f)
{
    const float s = f / (2.0f + f), z = s * s;
    float p = 1.0f / 13.0f;
    p = pol_fma(p, z, 1.0f / 11.0f);
    p = pol_fma(p, z, 1.0f / 9.0f);
    p = pol_fma(p, z, 1.0f / 7.0f);
    p = pol_fma(p, z, 1.0f / 5.0f);
    p = pol_fma(p, z, 1.0f / 3.0f);
    p = p * z;
    return pol_fma(-s, pol_fma(-2.0f, p, f), f);
}
MB_HD float pol_log_kf(int32_t k, float f)
{
    const float kf = (float)k;
    return pol_fma(kf, kLn2Hi, pol_fma(kf, kLn2Lo, pol_log1p_f(f)));
}

// log(x), x > 0 (x = 2^k m, m in [sqrt(1/2), sqrt(2)), f = m - 1 exact)
MB_HD float pol_log(float x)
{
    if (!(x == x)) return x;
    if (x < 0.0f) return u2f(0x7FC00000u);
    if (x == 0.0f) return u2f(0xFF800000u);
    uint32_t b = f2u(x);
    if (b >= 0x7F800000u) return x;
    int32_t k = 0;
    if (b < 0x00800000u) {   // subnormal: scaled up exactly first
        b = f2u(x * 33554432.0f);
        k = -25;
    }
    k += (int32_t)(b >> 23) - 127;
    float m = u2f((b & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421356f) {
        m = m * 0.5f;
        k += 1;
    }
    return pol_log_kf(k, m - 1.0f);
}

// log(1 + e) for e in [0, 1] with no rounding of 1 + e: f is e itself, or
// (e - 1) / 2 against k = 1 (both exact)
MB_HD float pol_log1p_01(float e)
{
    if (e < 0.41421356f) return pol_log1p_f(e);
    return pol_log_kf(1, (e - 1.0f) * 0.5f);
}

MB_HD float pol_tanh(float x)
{
    if (!(x == x)) return x;
    const float a = x < 0.0f ? -x : x;
    float t = 1.0f;
    if (a < 9.1f) {
        const float e = pol_expm1(a + a);
        t = e / (e + 2.0f);
    }
    return x < 0.0f ? -t : t;
}

MB_HD float pol_elu(float x)
{
    if (x > 0.0f || !(x == x)) return x;
    if (x < -18.0f) return -1.0f;
    return pol_expm1(x);
}

// log(sigmoid(x)) = min(x, 0) - log(1 + exp(-|x|))
MB_HD float pol_logsigmoid(float x)
{
    if (!(x == x)) return x;
    const float a = x < 0.0f ? -x : x;
    const float l = pol_log1p_01(pol_exp(-a));
    return x < 0.0f ? x - l : -l;
}

// sigmoid(x) = 1 / (1 + exp(-|x|)) for x >= 0, exp(-|x|) / (1 + exp(-|x|)) below:
// exactly 1 from where 1 + e rounds to 1, exactly 0 where pol_exp gives 0
MB_HD float pol_sigmoid(float x)
{
    if (!(x == x)) return x;
    const float a = x < 0.0f ? -x : x;
    const float e = pol_exp(-a), d = 1.0f + e;
    return x < 0.0f ? e / d : 1.0f / d;
}

// The gated memory head's new state (DESIGN.md "Gated memory head"): (1 - z) h
// + z c in two fmaf, exact at both ends -- z == 1 gives c, z == 0 gives h (a -0
// may come out as +0).
MB_HD float pol_gate_blend(float z, float c, float h) { return pol_fma(z, c, pol_fma(-z, h, h)); }
// Its point-wise backward from dh = d loss / d h': the gradients at the memory
// head's and the gate's pre-activations, and the direct term of d loss / d h.
// With z == 1 dpre_z and dh_direct are zeros, with z == 0 dpre_c is.
MB_HD void pol_gate_back(float dh, float z, float c, float h, float *dpre_c, float *dpre_z, float *dh_direct)
{
    const float omz = 1.0f - z;
    *dpre_c = (dh * z) * pol_fma(-c, c, 1.0f);
    *dpre_z = (dh * (c - h)) * (z * omz);
    *dh_direct = dh * omz;
}

MB_HD float pol_activation(int code, float x)
{
    switch (code) {
    case kActRelu: return x > 0.0f ? x : 0.0f;
    case kActLeaky: return x >= 0.0f ? x : 0.01f * x;
    case kActTanh: return pol_tanh(x);
    case kActElu: return pol_elu(x);
    case kActLogSigmoid: return pol_logsigmoid(x);
    case kActExp: return pol_exp(x);
    case kActLog: return pol_log(x);
    default: return x;
    }
}

// pol_activation and the gate head's sigmoid (code 8): what
// mbots_policy_activation evaluates.  Kept out of pol_activation's switch, which
// the trunk layers run on a code that is never 8.
MB_HD float pol_activation_any(int code, float x)
{
    return code == kActSigmoid ? pol_sigmoid(x) : pol_activation(code, x);
}

// the row's uniform: keyed by (seed, draw) and counted by (global world,
// species, index inside the (world, species) segment), so a shard ghost's rows
// draw what the next rank draws for them
MB_HD float pol_uniform(uint32_t seed, uint32_t draw, uint32_t gw, uint32_t species /* 1..4 */, uint32_t k)
{
    return u01(threefry2x32(seed, draw, gw, ((species - 1u) << 16) | k).x);
}

// softmax sampling of the six logits: returns the action, *logp its log
// probability.  Prefix sums are plain f32 adds in index order.
MB_HD int32_t pol_sample(const float z[kPolActions], float u, bool greedy, float *logp)
{
    float m = z[0];
    int32_t am = 0;
    for (int i = 1; i < kPolActions; ++i)
        if (z[i] > m) {
            m = z[i];
            am = i;
        }
    float c[kPolActions];
    float run = 0.0f;
    for (int i = 0; i < kPolActions; ++i) {
        run = run + pol_exp(z[i] - m);
        c[i] = run;
    }
    const float s = c[kPolActions - 1];
    int32_t a = am;
    if (!greedy) {
        const float us = u * s;
        a = kPolActions - 1;
        for (int i = kPolActions - 2; i >= 0; --i)
            if (us < c[i]) a = i;
    }
    float za = z[0];
    for (int i = 1; i < kPolActions; ++i)
        if (i == a) za = z[i];
    *logp = (za - m) - pol_log(s);
    return a;
}

// ---- the nets as the kernel and the CPU loops read them ----
// One Linear: the HIP path holds W in the B-fragment order of
// v_mfma_f32_16x16x4_f32 -- [kp / 4][nt][64] with lane l of k-step ks and
// column tile jt holding W[jt * 16 + (l & 15)][4 ks + (l >> 4)] -- and the
// bias padded to nt * 16; the CPU mode holds W as [nt * 16][kp] rows.  Pads
// are +0 on both sides.
struct PolLayer {
    float *w, *b;
    uint32_t in, out, kp, nt, act;
};
struct PolNet {
    uint32_t set, n_trunk, H, flags;   // flags: kPolMemoryIn
    uint32_t has_memory, gated, pad[2];   // gated: the gate head blends the memory head's output into HiddenState
    PolLayer trunk[kPolMaxTrunk], actor[2], critic[2], memory, gate;
};
struct PolNets {
    PolNet net[kNumSpecies];
};
// ---- policy groups (DESIGN.md "Device actor", "Policy groups"): contiguous
// ranges of global worlds, each with its own four nets ----
constexpr uint32_t kPolMaxGroups = 64;   // MBOTS_POLICY_MAX_GROUPS
// The groups as one manager sees them: the net table [G][4] (device memory in
// HIP mode; an entry with set == 0 has no net), each group's first local world
// clamped into [0, Wx] (first[G] = Wx, so group g owns the local worlds
// [first[g], first[g + 1])), and the group of the shard ghost's global world.
struct PolGroups {
    const PolNet *table;
    uint32_t G, ghost;
    uint32_t first[kPolMaxGroups + 1];
};
// the group of global world gw: the last g with starts[g] <= gw (starts[0] == 0)
MB_HD uint32_t pol_group_of(const uint32_t *starts, uint32_t G, uint32_t gw)
{
    uint32_t g = 0;
    while (g + 1u < G && starts[g + 1u] <= gw) ++g;
    return g;
}
// The table row at which local world lw's rows of species s (0..3) begin among
// the exported rows: row_base's entry, or past the last exported world the
// species' end.  Rows are ordered (species, world, slot), so [edge(first[g]),
// edge(first[g + 1])) is the one segment of (group g, species s).
MB_HD uint32_t pol_group_edge(const int32_t *row_base, uint32_t Wx, uint32_t lw, uint32_t s, uint32_t species_end)
{
    return lw < Wx ? (uint32_t)row_base[4u * lw + s] : species_end;
}

MB_HD size_t pol_w_floats(const PolLayer &l) { return (size_t)l.kp * l.nt * 16u; }
MB_HD size_t pol_b_floats(const PolLayer &l) { return (size_t)l.nt * 16u; }

// the repack / pad of one layer's weights at upload (src: [out][in] row-major;
// tr: src is the [in][out] matrix this layer is the transpose of)
// ld, off (tr only): src's row stride when not `out` (0: out), and the first of
// the `out` columns of it the layer takes
struct PolUpload {
    const float *w_src, *b_src;
    float *w_dst, *b_dst;
    uint32_t in, out, kp, nt, tr, ld, off;
};
struct PolUploads {
    PolUpload l[kPolLayers];
    uint32_t n;
};

// the 69 (with `hidden`: 85) input floats of a row from the table's columns, padded with +0 to kp
MB_HD void pol_row_input(float *x, const uint8_t *dep, const int8_t *sem, int32_t hp, const float *pos,
                         const float *sur, const float *hidden /* null: none */, uint32_t kp)
{
    for (int k = 0; k < kSensor; ++k) x[k] = (float)dep[k];
    x[32] = u2f((uint32_t)hp);
    x[33] = pos[0];
    x[34] = pos[1];
    for (int k = 0; k < kSensor; ++k) x[35 + k] = (float)sem[k];
    x[67] = sur[0];
    x[68] = sur[1];
    uint32_t n = kPolObs;
    if (hidden)
        for (int k = 0; k < kHidden; ++k) x[n++] = hidden[k];
    while (n < kp) x[n++] = 0.0f;
}

// ---- evaluate: act()'s chain on recorded (obs, action) rows, and its backward
// pass (DESIGN.md "Differentiable evaluate") ----
// The summation order of the parameter gradients: rows are cut into tiles of
// kPolGradRows, tile i belongs to accumulator i mod kPolGradAcc, an
// accumulator's chain runs over its rows in ascending order (continued from
// tile to tile), and the result is the accumulators added in ascending index.
constexpr uint32_t kPolGradRows = 64, kPolGradAcc = 256;
constexpr int kPolGradLayers = kPolMaxTrunk + 4;   // trunk, actor 2, critic 2 (the memory head takes no part)
// evaluate_sequences' gradients: those, then the memory head (slot kPolGradLayers)
constexpr int kPolSeqLayers = kPolGradLayers + 1;
// a gated net's: those, then the gate head (slot kPolSeqLayers)
constexpr int kPolGateLayers = kPolSeqLayers + 1;

// d activation / d input, from the layer's output y
MB_HD float pol_activation_grad(int code, float y)
{
    switch (code) {
    case kActRelu: return y > 0.0f ? 1.0f : 0.0f;
    case kActLeaky: return y >= 0.0f ? 1.0f : 0.01f;
    case kActTanh: return pol_fma(-y, y, 1.0f);
    case kActElu: return y > 0.0f ? 1.0f : y + 1.0f;
    case kActLogSigmoid: return 1.0f - pol_exp(y);
    default: return 1.0f;
    }
}

// One row's softmax head: logp of action a, the entropy, and (g_logp, g_entropy
// the upstream gradients) d loss / d logits.  m, the prefix sums and logp are
// pol_sample's own expressions.
MB_HD void pol_head(const float z[kPolActions], int32_t a, float g_logp, float g_entropy, float *logp,
                    float *entropy, float dz[kPolActions])
{
    float m = z[0];
    for (int i = 1; i < kPolActions; ++i)
        if (z[i] > m) m = z[i];
    float e[kPolActions];
    float s = 0.0f;
    for (int i = 0; i < kPolActions; ++i) {
        e[i] = pol_exp(z[i] - m);
        s = s + e[i];
    }
    const float ls = pol_log(s);
    float p[kPolActions], lp[kPolActions];
    float acc = 0.0f, la = 0.0f;
    for (int i = 0; i < kPolActions; ++i) {
        p[i] = e[i] / s;
        lp[i] = (z[i] - m) - ls;
        acc = pol_fma(p[i], lp[i], acc);
        if (i == a) la = lp[i];
    }
    const float ent = -acc;
    *logp = la;
    *entropy = ent;
    for (int i = 0; i < kPolActions; ++i) {
        const float t1 = g_logp * ((i == a ? 1.0f : 0.0f) - p[i]);
        const float t2 = (g_entropy * p[i]) * (lp[i] + ent);
        dz[i] = t1 - t2;
    }
}

// the rows an evaluate / its backward reads and writes (any output null: not wanted;
// any g_* null: zeros)
struct PolEvalIO {
    const float *obs, *hidden;   // [n][69], [n][16] (memory_in nets)
    const int32_t *action;       // [n]
    const float *g_logp, *g_value, *g_entropy;
    float *logp, *value, *entropy;
    uint64_t n;
};
// where a gradient call keeps its partial sums: nacc slabs of slab_floats
// each, layer l's dW at w[l] and db at b[l] inside a slab.  The device keeps dW
// in the C-fragment order of its 16 x 16 tiles, [nt][nkt][4][64] (nkt the
// 16-wide tiles of kp); the CPU mode as [out][in].
struct PolGradSlabs {
    float *base;
    uint64_t slab_floats;
    uint32_t w[kPolGateLayers], b[kPolGateLayers];
    uint32_t nacc;
};
// the gradients as the caller wants them ([out][in] / [out], null: not wanted), in
// the order trunk, actor, critic
struct PolGradOut {
    float *w[kPolGateLayers], *b[kPolGateLayers];
    uint32_t in[kPolGateLayers], out[kPolGateLayers], kp[kPolGateLayers];
    uint32_t n;   // slots in use: kPolGradLayers, kPolSeqLayers, or kPolGateLayers
};
MB_HD uint32_t pol_grad_nkt(uint32_t kp) { return (kp + 15u) >> 4; }

// ---- grouped evaluate: every (group, species) segment of a table through its
// own net in one forward and one backward call (DESIGN.md "Grouped evaluate") ----
// Segment e = 4 g + s is the rows [lo, hi) of `segments` [G][4][2], read on the
// device; its tiles, accumulators and chains are evaluate's, counted from lo.
constexpr uint32_t kPolEvalMaxSegs = 4u * kPolMaxGroups;
constexpr uint32_t kPolGroupWave = 8;    // segments whose backward shares a launch, its slabs and its stash
constexpr int kPolGroupUploads = 16;     // a net's 8 forward and 7 transposed layers, rounded up
// One net as a kernel argument carries it: every width follows from (n_trunk,
// H, flags), so the descriptors themselves are built on the device.
struct PolGroupSpec {
    uint64_t w_off;                     // floats from the workspace's start to the net's packed weights
    uint32_t n_trunk, H, flags, act;    // n_trunk == 0: the pair has no net; act: trunk layer l's code in byte l
    const float *w[kPolGradLayers], *b[kPolGradLayers];   // the caller's parameters (slots as PolGradOut's)
};
// The net's descriptors in the workspace: forward and transposed layers (as
// evaluate's plan lays them out) and where each layer's dW / db lie in a slab.
// (The grouped evaluate_sequences adds the memory head: its layer and slab slot
// kPolGradLayers, back.memory, and back.trunk[0] the H -> 16 layer of dh; a
// gated net's gate head is layer and slot kPolSeqLayers, with back.gate.)
struct PolGroupEntry {
    PolNet net, back;
    uint32_t sw[kPolGateLayers], sb[kPolGateLayers];
    uint32_t slab_floats, pad;
};
MB_HD float *pol_group_take(float *ws, uint64_t base, size_t &off, size_t floats)
{
    float *p = ws ? ws + base + off : nullptr;
    off += (floats + 63u) & ~size_t(63);
    return p;
}
// `e` (and, `up` not null, the `nup` repacks that fill its weights) from `s`;
// returns the floats the weights take from ws + s.w_off on.  seq: the net as
// evaluate_sequences runs it, with the memory head (parameters mw, mb) as layer
// kPolGradLayers and the transposed W0[:, 69:85] slice as back.trunk[0]; with
// kPolGate in s.flags the gate head (gw, gb) follows as layer kPolSeqLayers.
MB_HD size_t pol_group_entry(const PolGroupSpec &s, float *ws, PolGroupEntry &e, PolUpload *up,
                             int nup = kPolGroupUploads, bool seq = false, const float *mw = nullptr,
                             const float *mb = nullptr, const float *gw = nullptr, const float *gb = nullptr)
{
    e = PolGroupEntry{};
    size_t off = 0;
    int nu = 0;
    if (s.n_trunk) {
        const uint32_t H = s.H, in0 = (s.flags & kPolMemoryIn) ? (uint32_t)(kPolObs + kHidden) : (uint32_t)kPolObs;
        e.net.set = 1;
        e.net.n_trunk = s.n_trunk;
        e.net.H = H;
        e.net.flags = s.flags;
        e.net.has_memory = seq ? 1u : 0u;
        e.net.gated = seq && (s.flags & kPolGate) ? 1u : 0u;
        uint32_t slab = 0;
        for (int i = 0; i < (seq ? (e.net.gated ? kPolGateLayers : kPolSeqLayers) : kPolGradLayers); ++i) {
            PolLayer *f, *b;
            uint32_t in = H, out = H, act = 0;
            if (i == kPolSeqLayers) {
                f = &e.net.gate;
                b = &e.back.gate;
                out = (uint32_t)kHidden;
            } else if (i == kPolGradLayers) {
                f = &e.net.memory;
                b = &e.back.memory;
                out = (uint32_t)kHidden;
            } else if (i < kPolMaxTrunk) {
                if ((uint32_t)i >= s.n_trunk) continue;
                f = &e.net.trunk[i];
                b = i ? &e.back.trunk[i] : nullptr;
                if (i == 0) in = in0;
                act = (s.act >> (8 * i)) & 0xFFu;
            } else {
                const int h = i - kPolMaxTrunk;
                f = h < 2 ? &e.net.actor[h] : &e.net.critic[h - 2];
                b = h < 2 ? &e.back.actor[h] : &e.back.critic[h - 2];
                if (h == 1) out = (uint32_t)kPolActions;
                if (h == 3) out = 1u;
            }
            f->in = in;
            f->out = out;
            f->kp = pol_kp(in);
            f->nt = (out + 15u) / 16u;
            f->act = act;
            f->w = pol_group_take(ws, s.w_off, off, pol_w_floats(*f));
            f->b = pol_group_take(ws, s.w_off, off, pol_b_floats(*f));
            const float *pw = i == kPolSeqLayers ? gw : i == kPolGradLayers ? mw : s.w[i];
            const float *pb = i == kPolSeqLayers ? gb : i == kPolGradLayers ? mb : s.b[i];
            if (up) up[nu++] = PolUpload{pw, pb, f->w, f->b, in, out, f->kp, f->nt, 0u, 0u, 0u};
            if (seq && i == 0) {   // W0[:, 69:85] alone: dh_k
                PolLayer *d = &e.back.trunk[0];
                d->in = out;
                d->out = (uint32_t)kHidden;
                d->kp = (out + 7u) & ~7u;
                d->nt = 1u;
                d->w = pol_group_take(ws, s.w_off, off, pol_w_floats(*d));
                d->b = pol_group_take(ws, s.w_off, off, pol_b_floats(*d));
                if (up)
                    up[nu++] = PolUpload{pw, nullptr, d->w, d->b, d->in, d->out, d->kp, d->nt, 1u, in, (uint32_t)kPolObs};
            }
            if (b) {
                b->in = out;
                b->out = in;
                b->kp = (out + 7u) & ~7u;   // an even number of k-steps, as the layer kernel's paired loop takes
                b->nt = (in + 15u) / 16u;
                b->w = pol_group_take(ws, s.w_off, off, pol_w_floats(*b));
                b->b = pol_group_take(ws, s.w_off, off, pol_b_floats(*b));
                if (up) up[nu++] = PolUpload{pw, nullptr, b->w, b->b, b->in, b->out, b->kp, b->nt, 1u, 0u, 0u};
            }
            e.sw[i] = slab;
            slab += f->nt * pol_grad_nkt(f->kp) * 256u;
            e.sb[i] = slab;
            slab += f->nt * 16u;
        }
        e.slab_floats = slab;
    }
    if (up)
        for (; nu < nup; ++nu) up[nu] = PolUpload{};
    return off;
}
// the segments of one backward wave, and where their gradients go ([out][in] /
// [out], null: not wanted)
struct PolGroupWave {
    uint32_t seg[kPolGroupWave], n;
};
struct PolGroupGrads {
    float *w[kPolGroupWave][kPolGradLayers], *b[kPolGroupWave][kPolGradLayers];
};
// the specs a setup launch carries in its arguments
constexpr uint32_t kPolGroupChunk = 24;
struct PolGroupSpecs {
    PolGroupSpec s[kPolGroupChunk];
    uint32_t first, n;
};
static_assert(sizeof(PolGroupSpecs) + 64u <= 4096u, "a setup launch's specs travel as kernel arguments");

// ---- evaluate_sequences: the net along padded sequences with the memory
// head's output carried from step to step, and backpropagation through time
// (DESIGN.md "Backpropagation through HiddenState") ----
// Element (k, b) of the [L][B] batch is present iff k < length[b].  The
// parameter gradients' summation order: sequences in tiles of kPolGradRows
// columns, tile i into accumulator i mod kPolGradAcc, an accumulator's chain
// over its tiles ascending, inside a tile k from the tile's largest length - 1
// down to 0, inside a (tile, k) the 64 columns ascending.
struct PolSeqIO {
    const float *obs, *hidden0;      // [L][B][69], [B][16]
    const int32_t *action, *length;  // [L][B], [B]
    const float *g_logp, *g_value, *g_entropy;   // [L][B] (null: zeros)
    float *logp, *value, *entropy;   // [L][B], +0 where absent (null: not wanted)
    float *hidden;                   // [L][B][16]: the h_k each present element read
    uint32_t L;
    uint64_t B;
};
// floats of the per-accumulator h_k store of the backward pass
MB_HD size_t pol_seq_h_floats(uint32_t nacc, uint32_t L) { return (size_t)nacc * L * kPolGradRows * kHidden; }

// ---- grouped evaluate_sequences: every (group, species) net along its own
// columns of one padded batch (DESIGN.md "Grouped evaluate_sequences") ----
// Position p of segment e = 4 g + s, lo <= p < hi of `segments` [G][4][2],
// stands for column order[p] of the batch; tiles, accumulators and chains are
// evaluate_sequences', counted in positions from lo.
constexpr int kPolSeqGroupUploads = 20;   // a net's 10 forward and 10 transposed layers at most (the gate's included)
constexpr uint32_t kPolNoColumn = 0xFFFFFFFFu;   // an order entry outside [0, B): length 0, never read or written
struct PolSeqGroupSpec {
    PolGroupSpec s;
    const float *mw, *mb;   // the memory head's parameters
    const float *gw, *gb;   // the gate head's (s.flags has kPolGate)
};
constexpr uint32_t kPolSeqGroupChunk = 20;
struct PolSeqGroupSpecs {
    PolSeqGroupSpec s[kPolSeqGroupChunk];
    uint32_t first, n;
};
static_assert(sizeof(PolSeqGroupSpecs) + 64u <= 4096u, "a setup launch's specs travel as kernel arguments");
struct PolSeqGroupGrads {
    float *w[kPolGroupWave][kPolGateLayers], *b[kPolGroupWave][kPolGateLayers];
};
// the columns a host evaluate_sequences call runs: idx[0 .. n) of the batch's B
// (idx null: all B, in place)
struct PolSeqCols {
    const int32_t *idx;
    uint64_t n;
};
// sequence_segments' keys: net_id outside [0, nkeys) has no net
MB_HD bool pol_seq_key(int32_t id, uint32_t nkeys) { return id >= 0 && (uint32_t)id < nkeys; }

// ---- the update on the device (include/mbots.h "The update on the device";
// DESIGN.md "Device learner step"): the per-row and per-element arithmetic the
// kernels and the host loops share.  Plain + - * / and sqrt, one rounding each
// (the build never contracts), so a float32 restatement is exact.
constexpr uint32_t kLossAcc = 256;        // f64 accumulators of a (group, species) segment: row i into i mod 256

MB_HD float pol_loss_scale(int64_t rows) { return rows != 0 ? 1.0f / (float)rows : 0.0f; }

// a row's three upstream gradients and its share of the loss
MB_HD float pol_loss_row(float logp, float value, float entropy, float adv, float ret, float w, float value_coef,
                         float entropy_coef, float &g_logp, float &g_value, float &g_entropy)
{
    const float na = -adv;
    g_logp = na * w;
    const float d = value - ret;
    g_value = ((2.0f * value_coef) * d) * w;
    g_entropy = (-entropy_coef) * w;
    return ((na * logp + value_coef * (d * d)) - entropy_coef * entropy) * w;
}

struct PolLossIO {            // mbots_policy_a2c_loss's arguments
    const float *logp, *value, *entropy, *adv, *ret;
    const int32_t *end;       // null: every row kept
    const int32_t *segments;
    const int64_t *rows;
    float *g_logp, *g_value, *g_entropy;
    double *loss;
    uint64_t n;
    float value_coef, entropy_coef;
};

// ---- the sequence loss (mbots_policy_seq_a2c_loss): the padded [L, B] batches
// of the recurrent learners.  Element (k, b) is kept iff k < len, its table
// t0 + k lies before last_table (negative: no such bound) and it is not the
// last row of a lifeline a reset ended.  What is dropped is a suffix of the
// column, so the kept elements are k < pol_seq_kept(): the steps before the
// bound, less the reset's last row when the bound leaves it in.
MB_HD int32_t pol_seq_kept(int32_t len, int32_t t0, int32_t end, int32_t last_table)
{
    if (len <= 0) return 0;
    int64_t m = len;
    if (last_table >= 0) {
        const int64_t room = (int64_t)last_table - (int64_t)t0;
        m = room < 0 ? 0 : (room < m ? room : m);
    }
    if (end == 2 /* MBOTS_TRAJ_END_RESET */ && m == (int64_t)len) m -= 1;
    return (int32_t)m;
}

struct PolSeqLossIO {         // mbots_policy_seq_a2c_loss's (and mbots_policy_seq_group_rows') arguments
    const float *logp, *value, *entropy, *adv, *ret;   // [L, B]
    const int32_t *len, *t0, *end;                     // [B]
    const int32_t *order, *segments;
    const int64_t *rows;
    float *g_logp, *g_value, *g_entropy;
    double *loss;
    uint32_t L;
    uint64_t B;
    int32_t last_table;
    float value_coef, entropy_coef;
};

// ---- PPO on the device (include/mbots.h "PPO on the device"; DESIGN.md "PPO
// on the device"): the clipped surrogate, the clipped value loss, the advantage
// moments and the KL gate.  Plain + - * /, pol_exp and comparisons, one
// rounding each.
//
// The two-level order of every sum: element i of a (group, species) segment,
// counted from lo, belongs to chunk i / chunk and to f64 accumulator i mod 256
// of that chunk; a chunk's 256 accumulators are added in ascending index to +0,
// a segment's chunks in ascending index to +0, the four species in ascending
// order to +0, and that sum is added to the output slot.  An element is a row
// (kPpoChunk) or a column position of a sequence batch (kPpoSeqChunk), whose
// kept steps are added in ascending k.  Both chunks are multiples of kLossAcc.
// (The two chunks were chosen by measurement, profiles/policy_ppo_cost.json;
// scripts/policy_ppo_cost.py builds the other candidates with these macros.)
#ifndef MBOTS_PPO_CHUNK
#define MBOTS_PPO_CHUNK 4096
#endif
#ifndef MBOTS_PPO_SEQ_CHUNK
#define MBOTS_PPO_SEQ_CHUNK 512
#endif
constexpr uint32_t kPpoChunk = MBOTS_PPO_CHUNK;          // rows of a chunk
constexpr uint32_t kPpoSeqChunk = MBOTS_PPO_SEQ_CHUNK;   // column positions of a chunk
constexpr uint32_t kPpoStats = 6;         // per_row, pol * w, vl * w, entropy * w, kl, clipped
constexpr uint32_t kPpoMoments = 3;       // count, sum adv, sum adv^2
static_assert(kPpoChunk % kLossAcc == 0 && kPpoSeqChunk % kLossAcc == 0, "accumulator i mod 256 within a chunk");

// chunk partials of a call: [groups][4][chunks][slots] f64
MB_HD uint64_t pol_ppo_chunks(uint64_t n, uint32_t chunk) { return (n + chunk - 1u) / chunk; }
MB_HD uint64_t pol_ppo_bytes(uint64_t chunks, uint32_t groups)
{
    return (uint64_t)groups * 4u * chunks * kPpoStats * sizeof(double);
}

struct PpoCoef {
    float clip_lo, clip_hi;   // 1 - clip, 1 + clip, rounded once on the host
    float value_clip;         // read when vclip
    float value_coef, entropy_coef;
    uint32_t vclip;           // value_clip > 0 and old_value given
};
struct PpoNorm {
    float mean, inv;
};
// a group's normalisation constants from its moments (null: none)
MB_HD PpoNorm pol_ppo_norm(const double *m)
{
    PpoNorm N{0.0f, 1.0f};
    if (m == nullptr) return N;
    const double n = m[0], s1 = m[1], s2 = m[2];
    if (!(n >= 2.0)) return N;
    const double mu = s1 / n;
    double var = (s2 - s1 * mu) / (n - 1.0);
    if (!(var > 0.0)) var = 0.0;
#ifdef __HIP_DEVICE_COMPILE__
    const float sd = (float)sqrt(var);
#else
    const float sd = (float)std::sqrt(var);
#endif
    N.mean = (float)mu;
    N.inv = 1.0f / (sd + 1e-8f);
    return N;
}
// a kept row's share of the moments: the exact f64 values
MB_HD void pol_ppo_moment_add(double acc[kPpoMoments], float adv)
{
    acc[0] += 1.0;
    acc[1] += (double)adv;
    acc[2] += (double)adv * (double)adv;
}
// a NaN in the first argument stays: clamps and selections propagate it
MB_HD float pol_min(float a, float b) { return b < a ? b : a; }
MB_HD float pol_max(float a, float b) { return b > a ? b : a; }

// a row's three upstream gradients and its six shares of the statistics
MB_HD void pol_ppo_row(float logp, float value, float entropy, float old_logp, float old_value, float adv, float ret,
                       float w, bool normalise, const PpoNorm &N, const PpoCoef &C, float &g_logp, float &g_value,
                       float &g_entropy, float st[kPpoStats])
{
    const float A = normalise ? (adv - N.mean) * N.inv : adv;
    const float lr = logp - old_logp;
    const float ratio = pol_exp(lr);
    const float s1 = ratio * A;
    const float rc = pol_min(pol_max(ratio, C.clip_lo), C.clip_hi);
    const float s2 = rc * A;
    const float pol = -pol_min(s1, s2);
    g_logp = (s2 < s1 ? 0.0f : -s1) * w;   // a tie takes the unclipped branch
    const float d = value - ret, v1 = d * d;
    float vl = v1;
    if (C.vclip) {
        const float dv = value - old_value;
        const float dc = pol_min(pol_max(dv, -C.value_clip), C.value_clip);
        const float d2 = (old_value + dc) - ret, v2 = d2 * d2;
        vl = v2 > v1 ? v2 : v1;
        g_value = (C.value_coef * (v2 > v1 ? (dc == dv ? 2.0f * d2 : 0.0f) : 2.0f * d)) * w;
    } else {
        g_value = ((2.0f * C.value_coef) * d) * w;
    }
    g_entropy = (-C.entropy_coef) * w;
    st[0] = ((pol + C.value_coef * vl) - C.entropy_coef * entropy) * w;
    st[1] = pol * w;
    st[2] = vl * w;
    st[3] = entropy * w;
    st[4] = ((ratio - 1.0f) - lr) * w;
    st[5] = (rc != ratio ? 1.0f : 0.0f) * w;
}

struct PolPpoIO {             // mbots_policy_ppo_loss's (and mbots_policy_adv_moments') arguments
    const float *logp, *value, *entropy, *old_logp, *old_value, *adv, *ret;
    const int32_t *end;       // null: every row kept
    const int32_t *segments;
    const int64_t *rows;
    const double *moments;    // [G][3], null: raw advantages
    float *g_logp, *g_value, *g_entropy;
    double *out;              // stats [G][6] (or the moments [G][3] being summed)
    double *part;             // the workspace: chunk partials
    uint64_t n;
    uint32_t chunks;          // per segment: pol_ppo_chunks(n, kPpoChunk)
    PpoCoef C;
};
struct PolSeqPpoIO {          // mbots_policy_seq_ppo_loss's (and mbots_policy_seq_adv_moments') arguments
    const float *logp, *value, *entropy, *old_logp, *old_value, *adv, *ret;   // [L, B]
    const int32_t *len, *t0, *end;                                            // [B]
    const int32_t *order, *segments;
    const int64_t *rows;
    const double *moments;
    float *g_logp, *g_value, *g_entropy;
    double *out, *part;
    uint32_t L;
    uint64_t B;
    int32_t last_table;
    uint32_t chunks;          // per segment: pol_ppo_chunks(B, kPpoSeqChunk)
    PpoCoef C;
};
// the gate: the group's rows while it may still step, else 0 (a NaN KL closes it)
MB_HD int64_t pol_ppo_gate(int64_t gate, int64_t rows, double kl, double target_kl)
{
    return gate != 0 && rows != 0 && kl <= target_kl ? rows : 0;
}

struct AdamTensor {           // struct mbots_policy_adam_tensor
    float *param;
    const float *grad;
    float *m, *v;
    uint64_t n;
    uint32_t group;
};
struct AdamState {            // struct mbots_policy_adam_state
    uint32_t t;
    float b1t, b2t;
};
struct AdamCoef {
    float lr, beta1, beta2, om1, om2, eps;   // om: 1 - beta, rounded once on the host
};
MB_HD void pol_adam(float &p, float g, float &m, float &v, const AdamCoef &C, float c1, float c2)
{
    m = C.beta1 * m + C.om1 * g;
    v = C.beta2 * v + (C.om2 * g) * g;
#ifdef __HIP_DEVICE_COMPILE__
    const float root = sqrtf(v / c2);
#else
    const float root = std::sqrt(v / c2);
#endif
    p = p - (C.lr * (m / c1)) / (root + C.eps);
}
// One launch's tensors travel as kernel arguments: block b of the launch works
// on chunk b - first[i] (kAdamChunk elements) of tensor t[i], first[i] <= b <
// first[i + 1].
constexpr uint32_t kAdamTensors = 64, kAdamChunk = 1024;
struct AdamLaunch {
    AdamTensor t[kAdamTensors];
    uint32_t first[kAdamTensors + 1];
    uint32_t n;
};
static_assert(sizeof(AdamLaunch) + 128u <= 4096u, "a launch's tensor descriptors travel as kernel arguments");

// ---- mbots_policy_adam_clip: the global gradient norm of every group in a
// fixed order, then Adam on the clipped gradient and the decayed parameter.
// Accumulator j of a chunk: the exact f64 squares of its elements 4j .. 4j + 3
// (absent ones +0), added in ascending order; the 256 accumulators then fold
// as a tree, a_i += a_{i + h} for h = 128 .. 1.
MB_HD double pol_sq4(float a, float b, float c, float d)
{
    return (((double)a * (double)a + (double)b * (double)b) + (double)c * (double)c) + (double)d * (double)d;
}
// the workspace of a call over `chunks` chunks of `tensors` tensors with n > 0:
// [chunks] f64 chunk partials, [tensors] f64 tensor sums, [groups] f64 squared
// norms, [groups] f32 coef, [groups] u32 live (the group takes the step)
struct AdamClipWs {
    double *q, *tsum, *normsq;
    float *coef;
    uint32_t *live;
};
MB_HD uint64_t pol_adam_clip_bytes(uint64_t chunks, uint64_t tensors, uint32_t groups)
{
    return (chunks + tensors + groups) * sizeof(double) + (uint64_t)groups * (sizeof(float) + sizeof(uint32_t));
}
MB_HD AdamClipWs pol_adam_clip_ws(void *base, uint64_t chunks, uint64_t tensors, uint32_t groups)
{
    AdamClipWs W;
    W.q = static_cast<double *>(base);
    W.tsum = W.q + chunks;
    W.normsq = W.tsum + tensors;
    W.coef = reinterpret_cast<float *>(W.normsq + groups);
    W.live = reinterpret_cast<uint32_t *>(W.coef + groups);
    return W;
}
struct AdamClipCoef {
    float lw;         // lr * weight_decay, rounded once on the host
    float max_norm;
    uint32_t clip;    // max_norm is a positive finite number
    uint32_t decay;   // weight_decay != 0
};
// a group's norm and clip factor from its squared norm; false: the norm is not
// finite and the group is left untouched
MB_HD bool pol_clip_coef(double normsq, const AdamClipCoef &K, float &nrm, float &coef)
{
#ifdef __HIP_DEVICE_COMPILE__
    nrm = (float)sqrt(normsq);
#else
    nrm = (float)std::sqrt(normsq);
#endif
    coef = 1.0f;
    if (K.clip) {
        const float c = K.max_norm / (nrm + 1e-6f);
        if (c < 1.0f) coef = c;
    }
    return normsq - normsq == 0.0;   // neither inf nor NaN
}
MB_HD void pol_adam_clip(float &p, float g, float &m, float &v, const AdamCoef &C, const AdamClipCoef &K, float coef,
                         float c1, float c2)
{
    const float gc = K.clip ? g * coef : g;
    if (K.decay) p = p - K.lw * p;
    pol_adam(p, gc, m, v, C, c1, c2);
}
// a fold launch's tensors: chunk partials q[first[i] .. first[i + 1]) are tensor
// slot[i]'s, of group group[i]
struct AdamFold {
    uint32_t first[kAdamTensors + 1];
    uint32_t slot[kAdamTensors];
    uint32_t group[kAdamTensors];
    uint32_t n;
};

}  // namespace mbots
