/* A C99 host of the handle-free sequence calls of the C ABI (include/mbots.h,
 * "Training the memory head"), on host memory (device = -1): it builds a net
 * with a memory head, 70 padded sequences of up to 4 steps, actions and
 * upstream gradients from a fixed integer sequence, checks the refusals (a
 * short workspace, a net without a memory head or without
 * MBOTS_POLICY_MEMORY_IN, a length outside [0, L], a present action outside
 * 0..5 -- an absent one is not read), evaluates, takes the gradients, and
 * prints a digest of the four outputs and of every gradient, the memory head's
 * included.  tests/test_policy_seq_c_host.py builds it with gcc -std=c99
 * -pedantic -Werror and compares the digest with
 * PolicyNet.evaluate_sequences + backward(). */
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

#define H 32u
#define L 4u
#define B 70u

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

int main(void)
{
    struct mbots_policy_net net, bad;
    struct mbots_policy_grads grads;
    uint64_t d = 1469598103934665603ull, bytes = 0, small = 0;
    float *obs, *hidden0, *g_logp, *g_value, *g_entropy;
    static int32_t action[L * B], length[B];
    static float logp[L * B], value[L * B], entropy[L * B], hidden[L * B * 16u];
    void *ws;
    uint32_t i, full = B, shortest = B;
    int32_t keep;

    memset(&net, 0, sizeof net);
    memset(&grads, 0, sizeof grads);
    net.n_trunk = 2;
    net.flags = MBOTS_POLICY_MEMORY_IN;
    layer(&net.trunk[0], &grads.trunk[0], 85u, H, 3, 16384.0f);
    layer(&net.trunk[1], &grads.trunk[1], H, H, 4, 2048.0f);
    layer(&net.actor[0], &grads.actor[0], H, H, 0, 2048.0f);
    layer(&net.actor[1], &grads.actor[1], H, 6, 0, 1024.0f);
    layer(&net.critic[0], &grads.critic[0], H, H, 0, 2048.0f);
    layer(&net.critic[1], &grads.critic[1], H, 1, 0, 2048.0f);
    layer(&net.memory, &grads.memory, H, 16u, 0, 512.0f);
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
        if (length[i] == (int32_t)L) full = i;
        if (length[i] < (int32_t)L) shortest = i;
    }
    if (full == B || shortest == B) return 1;

    CHECK(mbots_policy_seq_workspace(&net, L, B, &bytes));
    CHECK(mbots_policy_seq_workspace(&net, 1, 1, &small));
    if (!bytes || small >= bytes) return 1;
    ws = malloc((size_t)bytes + 64u);
    if (!ws) return 2;
    ws = (void *)(((uintptr_t)ws + 63u) & ~(uintptr_t)63u);

    /* refusals */
    EXPECT(mbots_policy_seq_eval(&net, obs, action, length, hidden0, L, B, logp, value, entropy, hidden, ws, small, -1,
                                 NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_seq_eval(&net, obs, action, length, NULL, L, B, logp, value, entropy, hidden, ws, bytes, -1,
                                 NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_seq_grad(&net, obs, action, length, hidden0, L, B, g_logp, g_value, g_entropy, NULL, ws, bytes,
                                 -1, NULL), MBOTS_E_INVALID);
    bad = net;
    bad.memory.weight = NULL;
    EXPECT(mbots_policy_seq_workspace(&bad, L, B, &small), MBOTS_E_INVALID);
    bad = net;
    bad.flags = 0;
    bad.trunk[0].in = 69u;
    EXPECT(mbots_policy_seq_workspace(&bad, L, B, &small), MBOTS_E_INVALID);
    keep = length[3];
    length[3] = (int32_t)L + 1;
    EXPECT(mbots_policy_seq_eval(&net, obs, action, length, hidden0, L, B, logp, value, entropy, hidden, ws, bytes, -1,
                                 NULL), MBOTS_E_INVALID);
    length[3] = -1;
    EXPECT(mbots_policy_seq_grad(&net, obs, action, length, hidden0, L, B, g_logp, g_value, g_entropy, &grads, ws,
                                 bytes, -1, NULL), MBOTS_E_INVALID);
    length[3] = keep;
    keep = action[(L - 1u) * B + full];
    action[(L - 1u) * B + full] = 6;
    EXPECT(mbots_policy_seq_eval(&net, obs, action, length, hidden0, L, B, logp, value, entropy, hidden, ws, bytes, -1,
                                 NULL), MBOTS_E_INVALID);
    action[(L - 1u) * B + full] = keep;
    action[(L - 1u) * B + shortest] = -7;   /* absent: not read */

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
    for (i = 0; i < 16u * H; ++i)
        if (grads.memory.weight[i] != 0.0f) break;
    if (i == 16u * H) return 1;   /* the memory head received a gradient */
    /* no sequences: zero gradients */
    CHECK(mbots_policy_seq_grad(&net, NULL, NULL, NULL, NULL, L, 0, NULL, NULL, NULL, &grads, ws, bytes, -1, NULL));
    for (i = 0; i < 16u * H; ++i)
        if (grads.memory.weight[i] != 0.0f) return 1;
    if (grads.critic[1].bias[0] != 0.0f) return 1;

    printf("sequences %u digest %016llx\n", B, (unsigned long long)d);
    return 0;
}
