/* A C99 host of the gated memory head of the C ABI (include/mbots.h,
 * MBOTS_POLICY_GATE), in CPU mode: it builds one gated net from a fixed integer
 * sequence, checks the refusals (a gate without a memory head, without
 * MBOTS_POLICY_MEMORY_IN, of another input or output width, with a NULL weight;
 * a gate field full of garbage under a clear flag is not read), sets the net for
 * all four species of a small manager and acts three times, then runs 70 padded
 * sequences of up to 4 steps through mbots_policy_seq_eval and
 * mbots_policy_seq_grad, and prints a digest of act()'s outputs and columns and
 * one of the four sequence outputs and every gradient, the gate's last.
 * tests/test_policy_gate_c_host.py builds it with gcc -std=c99 -pedantic
 * -Werror and compares both digests with the Python API's. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mbots.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ < 0) {                                                           \
            fprintf(stderr, "%s: %d %s\n", #call, rc_, mbots_last_error());      \
            return 1;                                                            \
        }                                                                        \
    } while (0)
#define EXPECT(call, code)                                                       \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != (code)) {                                                     \
            fprintf(stderr, "%s: %d, expected %d\n", #call, rc_, (code));        \
            return 1;                                                            \
        }                                                                        \
    } while (0)
/* refused, and the message names the cause */
#define EXPECT_MSG(call, word)                                                   \
    do {                                                                         \
        EXPECT(call, MBOTS_E_INVALID);                                           \
        if (!strstr(mbots_last_error(), word)) {                                 \
            fprintf(stderr, "%s: \"%s\" lacks \"%s\"\n", #call, mbots_last_error(), word); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

#define H 32u
#define L 4u
#define B 70u
#define MAX_ROWS 1024u

static uint64_t fnv1a(const void *p, size_t n, uint64_t h)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

/* ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
static uint32_t lcg = 12345u;
static float *fill(size_t n, float div)
{
    float *p = (float *)malloc(n * sizeof(float));
    size_t i;
    if (!p) exit(2);
    for (i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        p[i] = (float)((int)((lcg >> 16) % 2001u) - 1000) / div;
    }
    return p;
}

static void layer(struct mbots_policy_layer *l, struct mbots_policy_grad_layer *g, uint32_t in, uint32_t out,
                  int32_t act, float div)
{
    l->in = in;
    l->out = out;
    l->act = act;
    l->weight = fill((size_t)in * out, div);
    l->bias = fill(out, 4096.0f);
    g->weight = (float *)malloc((size_t)in * out * sizeof(float));
    g->bias = (float *)malloc(out * sizeof(float));
    if (!g->weight || !g->bias) exit(2);
}

static uint64_t digest_layer(const struct mbots_policy_layer *l, const struct mbots_policy_grad_layer *g, uint64_t d)
{
    d = fnv1a(g->weight, (size_t)l->in * l->out * sizeof(float), d);
    return fnv1a(g->bias, l->out * sizeof(float), d);
}

static int32_t act_action[MAX_ROWS];
static float act_logp[MAX_ROWS], act_value[MAX_ROWS];

int main(void)
{
    struct mbots_policy_net net, bad;
    struct mbots_policy_grads grads;
    mbots_config cfg;
    mbots_handle *h = NULL;
    mbots_tensor ta, tm;
    uint64_t da = 1469598103934665603ull, d = 1469598103934665603ull, bytes = 0, plain = 0;
    float *obs, *hidden0, *g_logp, *g_value, *g_entropy;
    static int32_t action[L * B], length[B];
    static float logp[L * B], value[L * B], entropy[L * B], hidden[L * B * 16u];
    static float sig[4];
    static const float sig_x[4] = {200.0f, -200.0f, 0.0f, 1.0f};
    void *ws;
    uint32_t i, s, n = 0;
    int t;

    memset(&net, 0, sizeof net);
    memset(&grads, 0, sizeof grads);
    net.n_trunk = 2;
    net.flags = MBOTS_POLICY_MEMORY_IN | MBOTS_POLICY_GATE;
    layer(&net.trunk[0], &grads.trunk[0], 85u, H, 3, 16384.0f);
    layer(&net.trunk[1], &grads.trunk[1], H, H, 4, 2048.0f);
    layer(&net.actor[0], &grads.actor[0], H, H, 0, 2048.0f);
    layer(&net.actor[1], &grads.actor[1], H, 6, 0, 1024.0f);
    layer(&net.critic[0], &grads.critic[0], H, H, 0, 2048.0f);
    layer(&net.critic[1], &grads.critic[1], H, 1, 0, 2048.0f);
    layer(&net.memory, &grads.memory, H, 16u, 0, 512.0f);
    layer(&net.gate, &grads.gate, H, 16u, 0, 256.0f);
    obs = fill((size_t)L * B * 69u, 8.0f);
    hidden0 = fill((size_t)B * 16u, 1000.0f);
    g_logp = fill(L * B, 65536.0f);
    g_value = fill(L * B, 65536.0f);
    g_entropy = fill(L * B, 65536.0f);
    for (i = 0; i < L * B; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        action[i] = (int32_t)((lcg >> 16) % 6u);
    }
    for (i = 0; i < B; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        length[i] = (int32_t)((lcg >> 16) % (L + 1u));
    }

    /* the gate's sigmoid: activation code 8, exact at both ends */
    CHECK(mbots_policy_activation(8, sig_x, sig, 4, -1, NULL));
    if (sig[0] != 1.0f || sig[1] != 0.0f || sig[2] != 0.5f || !(sig[3] > 0.73f && sig[3] < 0.74f)) return 1;
    EXPECT(mbots_policy_activation(9, sig_x, sig, 4, -1, NULL), MBOTS_E_INVALID);

    /* refusals, each named */
    bad = net;
    bad.memory.weight = NULL;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "memory head");
    bad = net;
    bad.flags = MBOTS_POLICY_GATE;
    bad.trunk[0].in = 69u;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "MBOTS_POLICY_MEMORY_IN");
    bad = net;
    bad.gate.in = H + 16u;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "the gate head must be Linear(32, 16)");
    bad = net;
    bad.gate.out = 8u;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "the gate head must be Linear(32, 16)");
    bad = net;
    bad.gate.weight = NULL;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "the gate head: null weight");
    bad = net;
    bad.flags |= 4u;
    EXPECT_MSG(mbots_policy_seq_workspace(&bad, L, B, &bytes), "unknown policy net flags");
    /* without the flag the field is not read, whatever it holds */
    bad = net;
    bad.flags = MBOTS_POLICY_MEMORY_IN;
    memset(&bad.gate, 0xA5, sizeof bad.gate);
    CHECK(mbots_policy_seq_workspace(&bad, L, B, &plain));
    CHECK(mbots_policy_seq_workspace(&net, L, B, &bytes));
    if (!plain || bytes <= plain) return 1;   /* the gate's accumulators and layers */

    /* act(): the gated net for every species of a CPU-mode manager */
    memset(&cfg, 0, sizeof cfg);
    cfg.num_worlds = 6;
    cfg.rand_seed = 21;
    cfg.init_num_agents_per_world = 12;
    cfg.sensor_size = 32;
    cfg.agent_capacity = 128;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    CHECK(mbots_create(&cfg, &h));
    bad = net;
    bad.gate.out = 8u;
    EXPECT_MSG(mbots_policy_set(h, 1, &bad, NULL), "the gate head must be Linear(32, 16)");
    for (s = 1; s <= 4u; ++s) CHECK(mbots_policy_set(h, s, &net, NULL));
    for (t = 0; t < 3; ++t) {
        CHECK(mbots_policy_act(h, 0, act_action, act_logp, act_value, MAX_ROWS, NULL));
        CHECK(mbots_num_agents(h, &n));
        if (n > MAX_ROWS) return 1;
        CHECK(mbots_export(h, MBOTS_EXPORT_ACTION, &ta));
        CHECK(mbots_export(h, MBOTS_EXPORT_HIDDEN_STATE, &tm));
        da = fnv1a(act_action, n * sizeof(int32_t), da);
        da = fnv1a(act_logp, n * sizeof(float), da);
        da = fnv1a(act_value, n * sizeof(float), da);
        da = fnv1a(ta.data, (size_t)n * 6u * sizeof(int32_t), da);
        da = fnv1a(tm.data, (size_t)n * 16u * sizeof(float), da);
        CHECK(mbots_step(h, NULL));
    }
    CHECK(mbots_destroy(h));

    /* the sequences */
    ws = malloc((size_t)bytes + 64u);
    if (!ws) return 2;
    ws = (void *)(((uintptr_t)ws + 63u) & ~(uintptr_t)63u);
    EXPECT(mbots_policy_seq_eval(&net, obs, action, length, hidden0, L, B, logp, value, entropy, hidden, ws, plain, -1,
                                 NULL), MBOTS_E_INVALID);   /* the ungated net's workspace is too small */
    CHECK(mbots_policy_seq_eval(&net, obs, action, length, hidden0, L, B, logp, value, entropy, hidden, ws, bytes, -1,
                                NULL));
    d = fnv1a(logp, sizeof logp, d);
    d = fnv1a(value, sizeof value, d);
    d = fnv1a(entropy, sizeof entropy, d);
    d = fnv1a(hidden, sizeof hidden, d);
    CHECK(mbots_policy_seq_grad(&net, obs, action, length, hidden0, L, B, g_logp, g_value, g_entropy, &grads, ws, bytes,
                                -1, NULL));
    for (i = 0; i < 2u; ++i) d = digest_layer(&net.trunk[i], &grads.trunk[i], d);
    for (i = 0; i < 2u; ++i) d = digest_layer(&net.actor[i], &grads.actor[i], d);
    for (i = 0; i < 2u; ++i) d = digest_layer(&net.critic[i], &grads.critic[i], d);
    d = digest_layer(&net.memory, &grads.memory, d);
    d = digest_layer(&net.gate, &grads.gate, d);
    for (i = 0; i < 16u * H; ++i)
        if (grads.gate.weight[i] != 0.0f) break;
    if (i == 16u * H) return 1;   /* the gate received a gradient */
    /* no sequences: zero gradients, the gate's too */
    CHECK(mbots_policy_seq_grad(&net, NULL, NULL, NULL, NULL, L, 0, NULL, NULL, NULL, &grads, ws, bytes, -1, NULL));
    for (i = 0; i < 16u * H; ++i)
        if (grads.gate.weight[i] != 0.0f) return 1;
    if (grads.gate.bias[0] != 0.0f) return 1;

    printf("agents %u act %016llx sequences %u digest %016llx\n", n, (unsigned long long)da, B, (unsigned long long)d);
    return 0;
}
