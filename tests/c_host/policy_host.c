/* A C99 host of the device actor of the C ABI (include/mbots.h, "Acting on the
 * device"), in MBOTS_EXEC_CPU mode: it builds four small nets from a fixed
 * integer sequence, checks the refusals (act with a species' net missing, a bad
 * width, a bad activation code), sets the nets, acts and steps for a few
 * rounds -- sampled, greedy and without the write --, moves the draw counter
 * back to repeat a call, and prints a digest of every output and of the
 * Action / HiddenState columns after each call.
 * tests/test_policy_c_host.py builds it with gcc -std=c99 -pedantic -Werror and
 * compares the digest with the same calls made through madrona_bots. */
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

#define H 16u
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

/* weights: ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
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

static void layer(struct mbots_policy_layer *l, uint32_t in, uint32_t out, int32_t act, float div)
{
    l->in = in;
    l->out = out;
    l->act = act;
    l->weight = fill((size_t)in * out, div);
    l->bias = fill(out, 4096.0f);
}

static int32_t action[MAX_ROWS];
static float logp[MAX_ROWS], value[MAX_ROWS];

static int digest(mbots_handle *h, uint64_t *d)
{
    mbots_tensor a, m;
    uint32_t n = 0;
    CHECK(mbots_num_agents(h, &n));
    if (n > MAX_ROWS) return 1;
    CHECK(mbots_export(h, MBOTS_EXPORT_ACTION, &a));
    CHECK(mbots_export(h, MBOTS_EXPORT_HIDDEN_STATE, &m));
    *d = fnv1a(action, n * sizeof(int32_t), *d);
    *d = fnv1a(logp, n * sizeof(float), *d);
    *d = fnv1a(value, n * sizeof(float), *d);
    *d = fnv1a(a.data, (size_t)n * 6u * sizeof(int32_t), *d);
    *d = fnv1a(m.data, (size_t)n * 16u * sizeof(float), *d);
    return 0;
}

int main(void)
{
    mbots_config cfg;
    mbots_handle *h = NULL;
    struct mbots_policy_net net[4], bad;
    uint64_t d = 1469598103934665603ull;
    uint32_t s, draw = 99u, n = 0;
    int32_t first[MAX_ROWS];
    int t;

    memset(&cfg, 0, sizeof cfg);
    cfg.num_worlds = 6;
    cfg.rand_seed = 21;
    cfg.init_num_agents_per_world = 12;
    cfg.sensor_size = 32;
    cfg.world_offset = 5;
    cfg.agent_capacity = 128;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    CHECK(mbots_create(&cfg, &h));

    memset(net, 0, sizeof net);
    for (s = 0; s < 4u; ++s) {
        const int with_mem = (s & 1u) != 0;
        net[s].n_trunk = 2;
        net[s].flags = with_mem ? MBOTS_POLICY_MEMORY_IN : 0u;
        layer(&net[s].trunk[0], with_mem ? 85u : 69u, H, 3, 262144.0f);
        layer(&net[s].trunk[1], H, H, (int32_t)(s + 2u), 2048.0f);
        layer(&net[s].actor[0], H, H, 0, 2048.0f);
        layer(&net[s].actor[1], H, 6, 0, 1024.0f);
        layer(&net[s].critic[0], H, H, 0, 2048.0f);
        layer(&net[s].critic[1], H, 1, 0, 2048.0f);
        if (with_mem) layer(&net[s].memory, H, 16, 0, 2048.0f);
    }

    /* refusals */
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);
    for (s = 0; s < 3u; ++s) CHECK(mbots_policy_set(h, s + 1u, &net[s], NULL));
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);
    bad = net[3];
    bad.trunk[1].in = H + 1u;
    EXPECT(mbots_policy_set(h, 4, &bad, NULL), MBOTS_E_INVALID);
    bad = net[3];
    bad.trunk[0].act = 6;
    EXPECT(mbots_policy_set(h, 4, &bad, NULL), MBOTS_E_INVALID);
    bad = net[3];
    bad.actor[1].out = 5;
    EXPECT(mbots_policy_set(h, 4, &bad, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_set(h, 5, &net[3], NULL), MBOTS_E_INVALID);
    CHECK(mbots_policy_set(h, 4, &net[3], NULL));

    CHECK(mbots_policy_draw(h, 0, &draw));
    if (draw != 0u) return 1;
    for (t = 0; t < 4; ++t) {
        CHECK(mbots_policy_act(h, t == 2 ? MBOTS_ACT_GREEDY : 0u, action, logp, value, MAX_ROWS, NULL));
        if (digest(h, &d)) return 1;
        CHECK(mbots_step(h, NULL));
    }
    CHECK(mbots_policy_draw(h, 0, &draw));
    if (draw != 4u) return 1;

    /* the same table twice: another draw differs, the counter set back repeats */
    CHECK(mbots_num_agents(h, &n));
    CHECK(mbots_policy_act(h, MBOTS_ACT_NO_WRITE, action, logp, value, MAX_ROWS, NULL));
    if (digest(h, &d)) return 1;
    memcpy(first, action, n * sizeof(int32_t));
    CHECK(mbots_policy_act(h, MBOTS_ACT_NO_WRITE, action, logp, value, MAX_ROWS, NULL));
    if (memcmp(first, action, n * sizeof(int32_t)) == 0) {
        fprintf(stderr, "two draws gave the same actions\n");
        return 1;
    }
    draw = 4u;
    CHECK(mbots_policy_draw(h, 1, &draw));
    CHECK(mbots_policy_act(h, MBOTS_ACT_NO_WRITE, action, logp, value, MAX_ROWS, NULL));
    if (memcmp(first, action, n * sizeof(int32_t)) != 0) {
        fprintf(stderr, "the counter set back did not repeat the draw\n");
        return 1;
    }
    /* a weight refresh in place, then cleared: act is refused again */
    net[0].actor[1].weight = fill(H * 6u, 512.0f);
    CHECK(mbots_policy_set(h, 1, &net[0], NULL));
    CHECK(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL));
    if (digest(h, &d)) return 1;
    CHECK(mbots_policy_clear(h, 2));
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);

    printf("agents %u digest %016llx\n", n, (unsigned long long)d);
    CHECK(mbots_destroy(h));
    return 0;
}
