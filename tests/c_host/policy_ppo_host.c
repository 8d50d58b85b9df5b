/* A C99 host of PPO on the device of the C ABI (include/mbots.h, "PPO on the
 * device") on the host path (device == -1): 9000 recorded rows in the segments
 * of two groups -- one of 4097 rows, past a chunk of 4096 -- through
 * mbots_policy_adv_moments, mbots_policy_ppo_loss and mbots_policy_ppo_gate;
 * then 2000 padded sequences of up to 3 steps, sorted by mbots_policy_seq_order,
 * through mbots_policy_seq_group_rows, mbots_policy_seq_adv_moments and
 * mbots_policy_seq_ppo_loss.  Everything is built from a fixed integer
 * sequence.  It checks the refusals (a short workspace, clip outside (0, 1), a
 * negative value_coef, no groups) and prints the bits of the moments and the
 * statistics, the gates and FNV-1a checksums of the gradients.
 * tests/test_policy_ppo_c_host.py builds it with gcc -std=c99 -pedantic
 * -Werror, runs it and compares what it printed with the numpy restatement
 * (tests/policy_ppo_ref.py) on the same numbers.  It has no other dependency,
 * so it can also be built with -fsanitize=address,undefined and run alone. */
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
#define EXPECT(call, code, word)                                                 \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != (code) || !strstr(mbots_last_error(), (word))) {              \
            fprintf(stderr, "%s: %d (%s), expected %d with \"%s\"\n", #call, rc_, mbots_last_error(), (code),   \
                    (word));                                                     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

#define GROUPS 2u
#define N 9000u
#define L 3u
#define B 2000u
#define LAST_TABLE 4

/* ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
static uint32_t lcg = 13579u;
static uint32_t next(void)
{
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 16;
}
static float *fill(size_t n, float div)
{
    float *p = (float *)malloc((n ? n : 1u) * sizeof(float));
    size_t i;
    if (!p) exit(2);
    for (i = 0; i < n; ++i) p[i] = (float)((int)(next() % 2001u) - 1000) / div;
    return p;
}
static float *plus(const float *a, size_t n, float div)
{
    float *p = fill(n, div);
    size_t i;
    for (i = 0; i < n; ++i) p[i] = a[i] + p[i];
    return p;
}

static uint64_t fnv = 14695981039346656037ull;
static void sum(const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < bytes; ++i) fnv = (fnv ^ b[i]) * 1099511628211ull;
}
static void report(const char *name)
{
    printf(" %s %016llx", name, (unsigned long long)fnv);
    fnv = 14695981039346656037ull;
}
static void doubles(const char *name, const double *x, size_t n)
{
    size_t i;
    printf(" %s", name);
    for (i = 0; i < n; ++i) {
        uint64_t u;
        memcpy(&u, &x[i], sizeof u);
        printf(" %016llx", (unsigned long long)u);
    }
}

int main(void)
{
    static const int32_t segments[GROUPS][4][2] = {{{3, 4100}, {4100, 4100}, {4100, 4103}, {4103, 4500}},
                                                   {{4510, 4766}, {4766, 8000}, {8000, 8001}, {8001, 8950}}};
    int64_t rows[GROUPS] = {4497, 4440}, gate[GROUPS], seq_rows[GROUPS] = {0, 0};
    double moments[GROUPS][3], stats[GROUPS][6];
    int32_t *end, net_id[B], len[B], t0[B], send[B], order[B], seq_segments[GROUPS][4][2];
    float *logp, *value, *entropy, *old_logp, *old_value, *adv, *ret, *g_logp, *g_value, *g_entropy;
    uint64_t ws_bytes = 0, seq_bytes = 0;
    void *ws;
    uint32_t i;

    /* ---- the rows ---- */
    logp = fill(N, 500.0f), value = fill(N, 200.0f), entropy = fill(N, 1000.0f);
    old_logp = plus(logp, N, 4000.0f), old_value = plus(value, N, 1000.0f);
    adv = fill(N, 300.0f), ret = fill(N, 200.0f);
    g_logp = fill(N, 1.0f), g_value = fill(N, 1.0f), g_entropy = fill(N, 1.0f);   /* (garbage to overwrite) */
    end = (int32_t *)malloc(N * sizeof(int32_t));
    if (!end) return 2;
    for (i = 0; i < N; ++i) end[i] = (int32_t)(next() % 4u);
    memset(moments, 0, sizeof moments), memset(stats, 0, sizeof stats);

    EXPECT(mbots_policy_ppo_workspace(N, 0u, &ws_bytes), MBOTS_E_INVALID, "groups");
    CHECK(mbots_policy_ppo_workspace(N, GROUPS, &ws_bytes));
    CHECK(mbots_policy_ppo_workspace((uint64_t)L * B, GROUPS, &seq_bytes));
    ws = malloc((size_t)(ws_bytes > seq_bytes ? ws_bytes : seq_bytes));
    if (!ws) return 2;
    printf(" workspace %lu %lu", (unsigned long)ws_bytes, (unsigned long)seq_bytes);

    EXPECT(mbots_policy_adv_moments(adv, end, N, &segments[0][0][0], GROUPS, &moments[0][0], ws, 8u, -1, NULL),
           MBOTS_E_INVALID, "workspace");
    CHECK(mbots_policy_adv_moments(adv, end, N, &segments[0][0][0], GROUPS, &moments[0][0], ws, ws_bytes, -1, NULL));
    doubles("moments", &moments[0][0], GROUPS * 3u);

    EXPECT(mbots_policy_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, end, N, &segments[0][0][0], GROUPS,
                                 rows, &moments[0][0], 0.2f, 0.5f, 0.5f, 0.01f, g_logp, g_value, g_entropy, &stats[0][0],
                                 ws, 8u, -1, NULL),
           MBOTS_E_INVALID, "workspace");
    EXPECT(mbots_policy_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, end, N, &segments[0][0][0], GROUPS,
                                 rows, &moments[0][0], 1.0f, 0.5f, 0.5f, 0.01f, g_logp, g_value, g_entropy, &stats[0][0],
                                 ws, ws_bytes, -1, NULL),
           MBOTS_E_INVALID, "clip");
    EXPECT(mbots_policy_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, end, N, &segments[0][0][0], GROUPS,
                                 rows, &moments[0][0], 0.2f, 0.5f, -0.5f, 0.01f, g_logp, g_value, g_entropy, &stats[0][0],
                                 ws, ws_bytes, -1, NULL),
           MBOTS_E_INVALID, "value_coef");
    for (i = 0; i < GROUPS * 6u; ++i)
        if ((&stats[0][0])[i] != 0.0) {
            fprintf(stderr, "a refused call wrote statistics\n");
            return 1;
        }
    CHECK(mbots_policy_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, end, N, &segments[0][0][0], GROUPS,
                                rows, &moments[0][0], 0.2f, 0.5f, 0.5f, 0.01f, g_logp, g_value, g_entropy, &stats[0][0], ws,
                                ws_bytes, -1, NULL));
    doubles("stats", &stats[0][0], GROUPS * 6u);
    sum(g_logp, N * sizeof(float)), sum(g_value, N * sizeof(float)), sum(g_entropy, N * sizeof(float));
    report("gradients");

    /* the gate: a target between the two groups' KL closes the larger one; it stays closed */
    gate[0] = rows[0], gate[1] = rows[1];
    CHECK(mbots_policy_ppo_gate(&stats[0][0], rows, GROUPS, 0.5 * (stats[0][4] + stats[1][4]), gate, -1, NULL));
    printf(" gate %ld %ld", (long)gate[0], (long)gate[1]);
    CHECK(mbots_policy_ppo_gate(&stats[0][0], rows, GROUPS, 1e30, gate, -1, NULL));
    printf(" %ld %ld", (long)gate[0], (long)gate[1]);

    /* ---- the sequences ---- */
    free(logp), free(value), free(entropy), free(old_logp), free(old_value), free(adv), free(ret);
    free(g_logp), free(g_value), free(g_entropy);
    for (i = 0; i < B; ++i) net_id[i] = (int32_t)(next() % 10u);   /* 8 and 9: no net */
    for (i = 0; i < B; ++i) len[i] = (int32_t)(next() % (L + 1u));
    for (i = 0; i < B; ++i) t0[i] = (int32_t)(next() % 6u);
    for (i = 0; i < B; ++i) send[i] = (int32_t)(next() % 4u);
    for (i = 0; i < B; ++i)
        if (net_id[i] >= 2 && net_id[i] < 8 && i % 7u) net_id[i] = 1;   /* pair (0, 1): more than a chunk of 512 columns */
    logp = fill(L * B, 500.0f), value = fill(L * B, 200.0f), entropy = fill(L * B, 1000.0f);
    old_logp = plus(logp, L * B, 4000.0f), old_value = plus(value, L * B, 1000.0f);
    adv = fill(L * B, 300.0f), ret = fill(L * B, 200.0f);
    g_logp = fill(L * B, 1.0f), g_value = fill(L * B, 1.0f), g_entropy = fill(L * B, 1.0f);
    memset(moments, 0, sizeof moments), memset(stats, 0, sizeof stats);
    CHECK(mbots_policy_seq_order(net_id, B, GROUPS, order, &seq_segments[0][0][0], NULL, 0, -1, NULL));
    CHECK(mbots_policy_seq_group_rows(len, t0, send, B, order, &seq_segments[0][0][0], GROUPS, LAST_TABLE, seq_rows, -1,
                                      NULL));
    printf(" rows %ld %ld", (long)seq_rows[0], (long)seq_rows[1]);
    CHECK(mbots_policy_seq_adv_moments(adv, len, t0, send, L, B, order, &seq_segments[0][0][0], GROUPS, LAST_TABLE,
                                       &moments[0][0], ws, seq_bytes, -1, NULL));
    doubles("moments", &moments[0][0], GROUPS * 3u);
    EXPECT(mbots_policy_seq_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, len, t0, send, L, B, order,
                                     &seq_segments[0][0][0], GROUPS, LAST_TABLE, seq_rows, &moments[0][0], 0.0f, 0.5f,
                                     0.5f, 0.01f, g_logp, g_value, g_entropy, &stats[0][0], ws, seq_bytes, -1, NULL),
           MBOTS_E_INVALID, "clip");
    CHECK(mbots_policy_seq_ppo_loss(logp, value, entropy, old_logp, old_value, adv, ret, len, t0, send, L, B, order,
                                    &seq_segments[0][0][0], GROUPS, LAST_TABLE, seq_rows, &moments[0][0], 0.2f, 0.5f, 0.5f,
                                    0.01f, g_logp, g_value, g_entropy, &stats[0][0], ws, seq_bytes, -1, NULL));
    doubles("stats", &stats[0][0], GROUPS * 6u);
    sum(g_logp, L * B * sizeof(float)), sum(g_value, L * B * sizeof(float)), sum(g_entropy, L * B * sizeof(float));
    report("gradients");
    free(logp), free(value), free(entropy), free(old_logp), free(old_value), free(adv), free(ret);
    free(g_logp), free(g_value), free(g_entropy), free(end), free(ws);
    printf(" ok\n");
    return 0;
}
