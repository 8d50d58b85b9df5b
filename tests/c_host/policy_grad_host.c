/* A C99 host of the handle-free evaluate / gradient calls of the C ABI
 * (include/mbots.h, "Learning from what the actor did"), on host memory
 * (device = -1): it builds a net, 150 rows, actions and upstream gradients from a
 * fixed integer sequence, checks the refusals (a short workspace, an action
 * outside 0..5, a bad width, missing hidden rows), evaluates, takes the
 * gradients, and prints a digest of the three outputs and of every gradient.
 * tests/test_policy_grad_c_host.py builds it with gcc -std=c99 -pedantic
 * -Werror and compares the digest with PolicyNet.evaluate + backward(). */
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
#define N 150u

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

int main(void)
{
    struct mbots_policy_net net, bad;
    struct mbots_policy_grads grads;
    uint64_t d = 1469598103934665603ull, bytes = 0, small = 0;
    float *obs, *hidden, *g_logp, *g_value, *g_entropy;
    static int32_t action[N];
    static float logp[N], value[N], entropy[N];
    void *ws;
    uint32_t i;
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
    obs = fill((size_t)N * 69u, 8.0f);
    hidden = fill((size_t)N * 16u, 1000.0f);
    g_logp = fill(N, 65536.0f);
    g_value = fill(N, 65536.0f);
    g_entropy = fill(N, 65536.0f);
    for (i = 0; i < N; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        action[i] = (int32_t)((lcg >> 16) % 6u);
    }

    CHECK(mbots_policy_grad_workspace(&net, N, &bytes));
    CHECK(mbots_policy_grad_workspace(&net, 1, &small));
    if (!bytes || small >= bytes) return 1;
    ws = malloc((size_t)bytes + 64u);
    if (!ws) return 2;
    ws = (void *)(((uintptr_t)ws + 63u) & ~(uintptr_t)63u);

    /* refusals */
    EXPECT(mbots_policy_eval(&net, obs, hidden, action, N, logp, value, entropy, ws, small, -1, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_eval(&net, obs, NULL, action, N, logp, value, entropy, ws, bytes, -1, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_grad(&net, obs, hidden, action, N, g_logp, g_value, g_entropy, NULL, ws, bytes, -1, NULL),
           MBOTS_E_INVALID);
    bad = net;
    bad.actor[1].out = 5;
    EXPECT(mbots_policy_grad_workspace(&bad, N, &small), MBOTS_E_INVALID);
    EXPECT(mbots_policy_eval(&bad, obs, hidden, action, N, logp, value, entropy, ws, bytes, -1, NULL), MBOTS_E_INVALID);
    keep = action[7];
    action[7] = 6;
    EXPECT(mbots_policy_eval(&net, obs, hidden, action, N, logp, value, entropy, ws, bytes, -1, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_grad(&net, obs, hidden, action, N, g_logp, g_value, g_entropy, &grads, ws, bytes, -1, NULL),
           MBOTS_E_INVALID);
    action[7] = keep;

    CHECK(mbots_policy_eval(&net, obs, hidden, action, N, logp, value, entropy, ws, bytes, -1, NULL));
    d = fnv1a(logp, sizeof logp, d);
    d = fnv1a(value, sizeof value, d);
    d = fnv1a(entropy, sizeof entropy, d);
    CHECK(mbots_policy_grad(&net, obs, hidden, action, N, g_logp, g_value, g_entropy, &grads, ws, bytes, -1, NULL));
    for (i = 0; i < 2u; ++i) {
        d = fnv1a(grads.trunk[i].weight, (size_t)net.trunk[i].in * H * sizeof(float), d);
        d = fnv1a(grads.trunk[i].bias, H * sizeof(float), d);
    }
    for (i = 0; i < 2u; ++i) {
        d = fnv1a(grads.actor[i].weight, (size_t)net.actor[i].in * net.actor[i].out * sizeof(float), d);
        d = fnv1a(grads.actor[i].bias, net.actor[i].out * sizeof(float), d);
    }
    for (i = 0; i < 2u; ++i) {
        d = fnv1a(grads.critic[i].weight, (size_t)net.critic[i].in * net.critic[i].out * sizeof(float), d);
        d = fnv1a(grads.critic[i].bias, net.critic[i].out * sizeof(float), d);
    }
    /* no rows: zero gradients */
    CHECK(mbots_policy_grad(&net, NULL, NULL, NULL, 0, NULL, NULL, NULL, &grads, ws, bytes, -1, NULL));
    for (i = 0; i < 6u * H; ++i)
        if (grads.actor[1].weight[i] != 0.0f) return 1;
    if (grads.critic[1].bias[0] != 0.0f) return 1;

    printf("rows %u digest %016llx\n", N, (unsigned long long)d);
    return 0;
}
