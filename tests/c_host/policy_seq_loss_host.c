/* A C99 host of the recurrent update of the C ABI (include/mbots.h, "The
 * recurrent update on the device") on the host path (device == -1): 300 padded
 * sequences of up to 3 steps, built from a fixed integer sequence, sorted by
 * mbots_policy_seq_order into the segments of two groups, through
 * mbots_policy_seq_group_rows and mbots_policy_seq_a2c_loss; then two
 * mbots_policy_adam_clip steps (max_norm 1, weight decay 0.01) over two groups
 * of three tensors each, the second with a group whose rows are 0.  It checks
 * the refusals (an order entry named twice, a length past L, a short
 * workspace), that the idle group is untouched, and prints the kept totals,
 * the bits of the losses and norms and FNV-1a checksums of everything else the
 * calls wrote.  tests/test_policy_seq_loss_c_host.py builds it with gcc
 * -std=c99 -pedantic -Werror, runs it and compares what it printed with the
 * numpy restatement on the same numbers. */
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
#define L 3u
#define B 300u
#define TENSORS 3u
#define LAST_TABLE 4

/* ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
static uint32_t lcg = 24680u;
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
static unsigned long long bits64(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return (unsigned long long)u;
}
static unsigned bits32(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return (unsigned)u;
}

int main(void)
{
    static const uint64_t sizes[TENSORS] = {5u, 1024u, 2049u};
    int32_t net_id[B], len[B], t0[B], end[B], order[B], twice[B], segments[GROUPS][4][2];
    int64_t rows[GROUPS] = {0, 0}, second[GROUPS];
    double loss[GROUPS] = {0.0, 0.0};
    float grad_norm[GROUPS];
    struct mbots_policy_adam_tensor T[GROUPS * TENSORS];
    struct mbots_policy_adam_state state[GROUPS];
    float *logp, *value, *entropy, *adv, *ret, *g_logp, *g_value, *g_entropy, *idle;
    uint64_t ws_bytes = 0;
    void *ws;
    uint32_t i, g, k;
    int32_t keep;

    for (i = 0; i < B; ++i) net_id[i] = (int32_t)(next() % 10u);   /* 8 and 9: no net */
    for (i = 0; i < B; ++i) len[i] = (int32_t)(next() % (L + 1u));
    for (i = 0; i < B; ++i) t0[i] = (int32_t)(next() % 6u);
    for (i = 0; i < B; ++i) end[i] = (int32_t)(next() % 4u);
    logp = fill(L * B, 100.0f), value = fill(L * B, 50.0f), entropy = fill(L * B, 1000.0f);
    adv = fill(L * B, 200.0f), ret = fill(L * B, 50.0f);
    g_logp = fill(L * B, 1.0f), g_value = fill(L * B, 1.0f), g_entropy = fill(L * B, 1.0f);   /* (garbage to overwrite) */
    for (g = 0; g < GROUPS; ++g) {
        state[g].t = 0u;
        state[g].b1t = state[g].b2t = 1.0f;
        for (k = 0; k < TENSORS; ++k) {
            struct mbots_policy_adam_tensor *t = &T[g * TENSORS + k];
            t->n = sizes[k];
            t->group = g;
            t->param = fill((size_t)sizes[k], 1000.0f);
            t->grad = fill((size_t)sizes[k], 100.0f);
            t->m = (float *)calloc((size_t)sizes[k], sizeof(float));
            t->v = (float *)calloc((size_t)sizes[k], sizeof(float));
            if (!t->m || !t->v) return 2;
        }
    }

    CHECK(mbots_policy_seq_order(net_id, B, GROUPS, order, &segments[0][0][0], NULL, 0, -1, NULL));
    memcpy(twice, order, sizeof order);
    twice[segments[1][0][0] + 1] = twice[segments[1][0][0]];
    EXPECT(mbots_policy_seq_group_rows(len, t0, end, B, twice, &segments[0][0][0], GROUPS, LAST_TABLE, rows, -1, NULL),
           MBOTS_E_INVALID, "a second time");
    CHECK(mbots_policy_seq_group_rows(len, t0, end, B, order, &segments[0][0][0], GROUPS, LAST_TABLE, rows, -1, NULL));
    printf(" rows %ld %ld", (long)rows[0], (long)rows[1]);

    keep = len[order[0]];
    len[order[0]] = (int32_t)L + 1;
    EXPECT(mbots_policy_seq_a2c_loss(logp, value, entropy, adv, ret, len, t0, end, L, B, order, &segments[0][0][0],
                                     GROUPS, LAST_TABLE, rows, 0.5f, 0.01f, g_logp, g_value, g_entropy, loss, -1, NULL),
           MBOTS_E_INVALID, "length 4");
    len[order[0]] = keep;
    CHECK(mbots_policy_seq_a2c_loss(logp, value, entropy, adv, ret, len, t0, end, L, B, order, &segments[0][0][0], GROUPS,
                                    LAST_TABLE, rows, 0.5f, 0.01f, g_logp, g_value, g_entropy, loss, -1, NULL));
    printf(" loss %016llx %016llx", bits64(loss[0]), bits64(loss[1]));
    sum(g_logp, L * B * sizeof(float)), sum(g_value, L * B * sizeof(float)), sum(g_entropy, L * B * sizeof(float));
    report("gradients");

    CHECK(mbots_policy_adam_clip_workspace(T, GROUPS * TENSORS, GROUPS, &ws_bytes));
    ws = malloc((size_t)ws_bytes);
    if (!ws) return 2;
    EXPECT(mbots_policy_adam_clip(T, GROUPS * TENSORS, state, GROUPS, rows, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 1.0f,
                                  grad_norm, ws, ws_bytes - 1u, -1, NULL),
           MBOTS_E_INVALID, "workspace");
    CHECK(mbots_policy_adam_clip(T, GROUPS * TENSORS, state, GROUPS, rows, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 1.0f,
                                 grad_norm, ws, ws_bytes, -1, NULL));
    printf(" grad_norm %08x %08x", bits32(grad_norm[0]), bits32(grad_norm[1]));
    idle = (float *)malloc((size_t)sizes[2] * sizeof(float));
    if (!idle) return 2;
    memcpy(idle, T[TENSORS + 2u].param, (size_t)sizes[2] * sizeof(float));
    second[0] = rows[0];
    second[1] = 0;
    CHECK(mbots_policy_adam_clip(T, GROUPS * TENSORS, state, GROUPS, second, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 1.0f,
                                 grad_norm, ws, ws_bytes, -1, NULL));
    if (memcmp(idle, T[TENSORS + 2u].param, (size_t)sizes[2] * sizeof(float)) != 0 || state[1].t != 1u ||
        state[0].t != 2u) {
        fprintf(stderr, "the group with rows == 0 moved, or the step counts are %u %u\n", state[0].t, state[1].t);
        return 1;
    }
    for (i = 0; i < GROUPS * TENSORS; ++i) sum(T[i].param, (size_t)T[i].n * sizeof(float));
    report("param");
    for (i = 0; i < GROUPS * TENSORS; ++i) sum(T[i].m, (size_t)T[i].n * sizeof(float));
    report("m");
    for (i = 0; i < GROUPS * TENSORS; ++i) sum(T[i].v, (size_t)T[i].n * sizeof(float));
    report("v");
    for (g = 0; g < GROUPS; ++g) sum(&state[g].t, 4u), sum(&state[g].b1t, 4u), sum(&state[g].b2t, 4u);
    report("state");
    printf(" ok\n");
    return 0;
}
