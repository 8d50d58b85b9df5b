/* A C99 host of the policy groups of the C ABI (include/mbots.h, "Acting on
 * the device": mbots_policy_groups, mbots_policy_num_groups,
 * mbots_policy_set_group, mbots_policy_clear_group, mbots_policy_segments), in
 * MBOTS_EXEC_CPU mode: a shard of six worlds at world_offset 5 with its ghost,
 * cut into four groups by global index -- the last owns the ghost world alone
 * --, each with four nets of its own (two architectures, alternating) built
 * from a fixed integer sequence.  It checks the refusals (starts that do not
 * begin at 0, starts not ascending, 65 starts, a group or species out of range,
 * act with a needed net missing), acts and steps for a few rounds, and prints a
 * digest of the segments, of every output and of the Action / HiddenState
 * columns after each call.  tests/test_policy_groups_c_host.py builds it with
 * gcc -std=c99 -pedantic -Werror and compares the digest with the same calls
 * made through madrona_bots. */
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

#define MAX_ROWS 1024u
#define GROUPS 4u

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
static uint32_t lcg = 777u;
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

static int32_t action[MAX_ROWS], seg[GROUPS * 4u * 2u];
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
    static const uint32_t starts[GROUPS] = {0u, 7u, 9u, 11u};   /* worlds 5 6 | 7 8 | 9 10 | the ghost, 11 */
    static const uint32_t not_zero[2] = {1u, 2u}, not_ascending[3] = {0u, 5u, 5u};
    uint32_t many[MBOTS_POLICY_MAX_GROUPS + 1], got[MBOTS_POLICY_MAX_GROUPS];
    mbots_config cfg;
    mbots_handle *h = NULL;
    struct mbots_policy_net net[GROUPS][4];
    uint64_t d = 1469598103934665603ull;
    uint32_t g, s, n = 0, ng = 0;
    int t;

    memset(&cfg, 0, sizeof cfg);
    cfg.num_worlds = 6;
    cfg.rand_seed = 21;
    cfg.init_num_agents_per_world = 12;
    cfg.sensor_size = 32;
    cfg.world_offset = 5;
    cfg.agent_capacity = 128;
    cfg.flags = MBOTS_FLAG_SHARD_GHOST;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    CHECK(mbots_create(&cfg, &h));

    memset(net, 0, sizeof net);
    for (g = 0; g < GROUPS; ++g)
        for (s = 0; s < 4u; ++s) {
            const int big = (g & 1u) != 0;   /* H = 32, one trunk layer, memory head and memory_in */
            const uint32_t H = big ? 32u : 16u;
            struct mbots_policy_net *q = &net[g][s];
            q->n_trunk = big ? 1u : 2u;
            q->flags = big ? MBOTS_POLICY_MEMORY_IN : 0u;
            layer(&q->trunk[0], big ? 85u : 69u, H, 3, 262144.0f);
            if (!big) layer(&q->trunk[1], H, H, (int32_t)(s + 2u), 2048.0f);
            layer(&q->actor[0], H, H, 0, 2048.0f);
            layer(&q->actor[1], H, 6, 0, 1024.0f);
            layer(&q->critic[0], H, H, 0, 2048.0f);
            layer(&q->critic[1], H, 1, 0, 2048.0f);
            if (big) layer(&q->memory, H, 16, 0, 2048.0f);
        }

    /* a manager starts with one group */
    CHECK(mbots_policy_num_groups(h, &ng, got));
    if (ng != 1u || got[0] != 0u) return 1;
    CHECK(mbots_policy_segments(h, seg, NULL));
    CHECK(mbots_num_agents(h, &n));
    if (seg[0] != 0 || seg[7] != (int32_t)n) return 1;

    /* refusals */
    for (g = 0; g <= MBOTS_POLICY_MAX_GROUPS; ++g) many[g] = g;
    EXPECT(mbots_policy_groups(h, not_zero, 2), MBOTS_E_INVALID);
    EXPECT(mbots_policy_groups(h, not_ascending, 3), MBOTS_E_INVALID);
    EXPECT(mbots_policy_groups(h, many, MBOTS_POLICY_MAX_GROUPS + 1), MBOTS_E_INVALID);
    CHECK(mbots_policy_groups(h, many, MBOTS_POLICY_MAX_GROUPS));
    CHECK(mbots_policy_groups(h, starts, GROUPS));
    CHECK(mbots_policy_num_groups(h, &ng, NULL));
    CHECK(mbots_policy_num_groups(h, &ng, got));
    if (ng != GROUPS || memcmp(got, starts, sizeof starts) != 0) return 1;
    EXPECT(mbots_policy_set_group(h, GROUPS, 1, &net[0][0], NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_set_group(h, 0, 5, &net[0][0], NULL), MBOTS_E_INVALID);
    EXPECT(mbots_policy_clear_group(h, GROUPS, 1), MBOTS_E_INVALID);
    for (g = 0; g < GROUPS; ++g)
        for (s = 0; s < 4u; ++s)
            if (g != 3u || s != 1u) CHECK(mbots_policy_set_group(h, g, s + 1u, &net[g][s], NULL));
    /* (group 3 owns the ghost world only: its nets are needed all the same) */
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);
    if (!strstr(mbots_last_error(), "group 3 species 2")) return 1;
    CHECK(mbots_policy_set_group(h, 3, 2, &net[3][1], NULL));

    for (t = 0; t < 4; ++t) {
        CHECK(mbots_policy_segments(h, seg, NULL));
        d = fnv1a(seg, sizeof seg, d);
        CHECK(mbots_policy_act(h, t == 2 ? MBOTS_ACT_GREEDY : 0u, action, logp, value, MAX_ROWS, NULL));
        if (digest(h, &d)) return 1;
        CHECK(mbots_step(h, NULL));
    }
    /* group 3 has no exported row */
    CHECK(mbots_policy_segments(h, seg, NULL));
    for (s = 0; s < 4u; ++s)
        if (seg[(3u * 4u + s) * 2u] != seg[(3u * 4u + s) * 2u + 1u]) return 1;

    /* mbots_policy_set without a group: every group's species 1 */
    CHECK(mbots_policy_set(h, 1, &net[2][0], NULL));
    CHECK(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL));
    if (digest(h, &d)) return 1;
    /* one net cleared: act is refused; the starts in place again keep the others */
    CHECK(mbots_policy_clear_group(h, 2, 3));
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);
    CHECK(mbots_policy_groups(h, starts, GROUPS));
    CHECK(mbots_policy_set_group(h, 2, 3, &net[2][2], NULL));
    CHECK(mbots_policy_act(h, MBOTS_ACT_NO_WRITE, action, logp, value, MAX_ROWS, NULL));
    if (digest(h, &d)) return 1;
    /* back to one group: every net is gone */
    CHECK(mbots_policy_groups(h, NULL, 0));
    CHECK(mbots_policy_num_groups(h, &ng, got));
    if (ng != 1u || got[0] != 0u) return 1;
    EXPECT(mbots_policy_act(h, 0, action, logp, value, MAX_ROWS, NULL), MBOTS_E_INVALID);

    CHECK(mbots_num_agents(h, &n));
    printf("agents %u digest %016llx\n", n, (unsigned long long)d);
    CHECK(mbots_destroy(h));
    return 0;
}
