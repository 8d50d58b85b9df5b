/* A C99 host of the device learner step of the C ABI (include/mbots.h, "The
 * update on the device") on the host path (device == -1): rows in the segments
 * of two groups, built from a fixed integer sequence, through
 * mbots_policy_group_rows and mbots_policy_a2c_loss; then two mbots_policy_adam
 * steps over two groups of ten tensors each (the tensors of an H = 16 net), the
 * second with a group whose rows are 0.  It checks the refusals (overlapping
 * segments, a tensor of a group past `groups`, a NULL state), that the idle
 * group is untouched, and prints FNV-1a checksums of everything the calls
 * wrote.  tests/test_policy_adam_c_host.py builds it with gcc -std=c99
 * -pedantic -Werror, runs it and compares the checksums with the Python
 * wrappers' results on the same numbers. */
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
#define N 600u
#define TENSORS 10u

/* ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
static uint32_t lcg = 97531u;
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

int main(void)
{
    static const uint64_t sizes[TENSORS] = {16u * 69u, 16u, 256u, 16u, 96u, 6u, 256u, 16u, 16u, 1u};
    int32_t segments[GROUPS][4][2] = {{{0, 257}, {257, 257}, {257, 258}, {258, 300}},
                                      {{310, 400}, {400, 400}, {400, 600}, {600, 600}}};
    int32_t overlap[GROUPS][4][2] = {{{0, 257}, {256, 257}, {257, 258}, {258, 300}},
                                     {{310, 400}, {400, 400}, {400, 600}, {600, 600}}};
    int64_t rows[GROUPS] = {0, 0}, second[GROUPS];
    double loss[GROUPS] = {0.0, 0.0};
    struct mbots_policy_adam_tensor T[GROUPS * TENSORS];
    struct mbots_policy_adam_state state[GROUPS];
    float *logp = fill(N, 100.0f), *value = fill(N, 50.0f), *entropy = fill(N, 1000.0f);
    float *adv = fill(N, 200.0f), *ret = fill(N, 50.0f);
    float *g_logp = fill(N, 1.0f), *g_value = fill(N, 1.0f), *g_entropy = fill(N, 1.0f);   /* (garbage to overwrite) */
    float *idle;
    int32_t end[N];
    uint32_t i, g, k;

    for (i = 0; i < N; ++i) end[i] = (int32_t)(next() % 4u);
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

    CHECK(mbots_policy_group_rows(&segments[0][0][0], GROUPS, rows, -1, NULL));
    if (rows[0] != 300 || rows[1] != 290) {
        fprintf(stderr, "group rows %ld %ld\n", (long)rows[0], (long)rows[1]);
        return 1;
    }
    EXPECT(mbots_policy_a2c_loss(logp, value, entropy, adv, ret, end, N, &overlap[0][0][0], GROUPS, rows, 0.5f, 0.01f,
                                 g_logp, g_value, g_entropy, loss, -1, NULL),
           MBOTS_E_INVALID, "overlap");
    CHECK(mbots_policy_a2c_loss(logp, value, entropy, adv, ret, end, N, &segments[0][0][0], GROUPS, rows, 0.5f, 0.01f,
                                g_logp, g_value, g_entropy, loss, -1, NULL));
    for (i = 300; i < 310; ++i)
        if (g_logp[i] != 0.0f || g_value[i] != 0.0f || g_entropy[i] != 0.0f) {
            fprintf(stderr, "row %u of no segment is not zero\n", i);
            return 1;
        }
    sum(g_logp, N * sizeof(float)), sum(g_value, N * sizeof(float)), sum(g_entropy, N * sizeof(float));
    report("gradients");
    sum(loss, sizeof(loss));
    report("loss");

    T[3].group = GROUPS;
    EXPECT(mbots_policy_adam(T, GROUPS * TENSORS, state, GROUPS, rows, 1e-3f, 0.9f, 0.999f, 1e-8f, -1, NULL),
           MBOTS_E_INVALID, "group");
    T[3].group = 0u;
    EXPECT(mbots_policy_adam(T, GROUPS * TENSORS, NULL, GROUPS, rows, 1e-3f, 0.9f, 0.999f, 1e-8f, -1, NULL),
           MBOTS_E_INVALID, "null");
    CHECK(mbots_policy_adam(T, GROUPS * TENSORS, state, GROUPS, rows, 1e-3f, 0.9f, 0.999f, 1e-8f, -1, NULL));
    idle = (float *)malloc((size_t)sizes[0] * sizeof(float));
    if (!idle) return 2;
    memcpy(idle, T[TENSORS].param, (size_t)sizes[0] * sizeof(float));
    second[0] = rows[0];
    second[1] = 0;
    CHECK(mbots_policy_adam(T, GROUPS * TENSORS, state, GROUPS, second, 1e-3f, 0.9f, 0.999f, 1e-8f, -1, NULL));
    if (memcmp(idle, T[TENSORS].param, (size_t)sizes[0] * sizeof(float)) != 0 || state[1].t != 1u || state[0].t != 2u) {
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
