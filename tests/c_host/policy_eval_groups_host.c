/* A C99 host of the grouped evaluate of the C ABI (include/mbots.h, "Every
 * group's nets in one call") on the host path (device == -1): two groups of
 * nets built from a fixed integer sequence -- different widths and depths, one
 * pair without a net (n_trunk == 0) --, rows in segments that leave gaps, and
 * the three calls.  It checks the refusals (a workspace that is too small, a
 * NULL `out`, NULL segments, overlapping and out-of-range segments, a missing
 * hidden), then that every output and every gradient equals, byte for byte,
 * what mbots_policy_eval / mbots_policy_grad give on each segment's rows alone,
 * and that the rows of no net are +0.
 * tests/test_policy_eval_groups_c_host.py builds it with gcc -std=c99 -pedantic
 * -Werror and runs it. */
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
#define SEGS (4u * GROUPS)
#define N 400u

/* ((x_n >> 16) % 2001 - 1000) / div, x_{n+1} = 1664525 x_n + 1013904223 (mod 2^32) */
static uint32_t lcg = 2468u;
static float *fill(size_t n, float div)
{
    float *p = (float *)malloc((n ? n : 1u) * sizeof(float));
    size_t i;
    if (!p) exit(2);
    for (i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        p[i] = (float)((int)((lcg >> 16) % 2001u) - 1000) / div;
    }
    return p;
}

static void layer(struct mbots_policy_layer *l, struct mbots_policy_grad_layer *a, struct mbots_policy_grad_layer *b,
                  uint32_t in, uint32_t out, int32_t act, float div)
{
    l->in = in;
    l->out = out;
    l->act = act;
    l->weight = fill((size_t)in * out, div);
    l->bias = fill(out, 4096.0f);
    a->weight = fill((size_t)in * out, 1.0f);   /* (garbage the calls overwrite) */
    a->bias = fill(out, 1.0f);
    b->weight = fill((size_t)in * out, 1.0f);
    b->bias = fill(out, 1.0f);
}

static int same(const float *a, const float *b, size_t n, const char *what, unsigned e)
{
    if (memcmp(a, b, n * sizeof(float)) != 0) {
        fprintf(stderr, "segment %u: %s differs from the per-net call\n", e, what);
        return 0;
    }
    return 1;
}

/* a layer's two gradients of the grouped call against the per-net call's */
static int same_layer(const struct mbots_policy_layer *l, const struct mbots_policy_grad_layer *a,
                      const struct mbots_policy_grad_layer *b, const char *what, unsigned e)
{
    return same(a->weight, b->weight, (size_t)l->in * l->out, what, e) && same(a->bias, b->bias, l->out, what, e);
}

int main(void)
{
    static struct mbots_policy_net nets[SEGS];
    static struct mbots_policy_grads grouped[SEGS], single[SEGS];
    /* (group 0 species 3 has no net; group 1 species 2 is empty) */
    static const int32_t seg_ok[SEGS][2] = {{3, 68},    {68, 69},   {200, 230}, {69, 133},
                                            {133, 196}, {260, 260}, {260, 389}, {389, 397}};
    int32_t seg[SEGS][2];
    float *obs = fill((size_t)N * 69u, 8.0f), *hidden = fill((size_t)N * 16u, 1000.0f);
    float *g[3], *out[3], *ref[3];
    static int32_t action[N];
    uint64_t bytes = 0, one = 0;
    void *ws;
    unsigned e, i, k;

    for (i = 0; i < N; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        action[i] = (int32_t)((lcg >> 16) % 6u);
    }
    for (k = 0; k < 3u; ++k) {
        g[k] = fill(N, 65536.0f);
        out[k] = fill(N, 1.0f);
        ref[k] = fill(N, 1.0f);
    }
    memset(nets, 0, sizeof nets);
    memset(grouped, 0, sizeof grouped);
    memset(single, 0, sizeof single);
    for (e = 0; e < SEGS; ++e) {
        const uint32_t big = e >= 4u, H = big ? 48u : 16u, T = big ? 3u : 1u + (e & 1u);
        uint32_t l;
        if (e == 2u) continue;
        nets[e].n_trunk = T;
        nets[e].flags = big ? MBOTS_POLICY_MEMORY_IN : 0u;
        for (l = 0; l < T; ++l)
            layer(&nets[e].trunk[l], &grouped[e].trunk[l], &single[e].trunk[l], l ? H : (big ? 85u : 69u), H,
                  (int32_t)(1u + (e + l) % 5u), l ? 2048.0f : 262144.0f);
        layer(&nets[e].actor[0], &grouped[e].actor[0], &single[e].actor[0], H, H, 0, 2048.0f);
        layer(&nets[e].actor[1], &grouped[e].actor[1], &single[e].actor[1], H, 6, 0, 1024.0f);
        layer(&nets[e].critic[0], &grouped[e].critic[0], &single[e].critic[0], H, H, 0, 2048.0f);
        layer(&nets[e].critic[1], &grouped[e].critic[1], &single[e].critic[1], H, 1, 0, 2048.0f);
    }
    memcpy(seg, seg_ok, sizeof seg);

    CHECK(mbots_policy_groups_workspace(nets, GROUPS, N, &bytes));
    ws = malloc(bytes);
    if (!ws || !bytes) return 2;

    /* refusals */
    EXPECT(mbots_policy_groups_workspace(nets, 0, N, &bytes), MBOTS_E_INVALID, "groups");
    EXPECT(mbots_policy_groups_workspace(nets, 65, N, &bytes), MBOTS_E_INVALID, "groups");
    EXPECT(mbots_policy_eval_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, out[0], out[1], out[2], ws,
                                    bytes - 1u, -1, NULL), MBOTS_E_INVALID, "workspace");
    EXPECT(mbots_policy_grad_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, g[0], g[1], g[2], NULL, ws,
                                    bytes, -1, NULL), MBOTS_E_INVALID, "null");
    EXPECT(mbots_policy_eval_groups(nets, GROUPS, NULL, obs, hidden, action, N, out[0], out[1], out[2], ws, bytes, -1,
                                    NULL), MBOTS_E_INVALID, "segments");
    EXPECT(mbots_policy_eval_groups(nets, GROUPS, &seg[0][0], obs, NULL, action, N, out[0], out[1], out[2], ws, bytes,
                                    -1, NULL), MBOTS_E_INVALID, "hidden");
    seg[3][0] = 67;   /* into group 0 species 1 */
    EXPECT(mbots_policy_eval_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, out[0], out[1], out[2], ws, bytes,
                                    -1, NULL), MBOTS_E_INVALID, "group 0 species 1 and group 0 species 4 overlap");
    memcpy(seg, seg_ok, sizeof seg);
    seg[7][1] = (int32_t)N + 1;
    EXPECT(mbots_policy_grad_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, g[0], g[1], g[2], grouped, ws,
                                    bytes, -1, NULL), MBOTS_E_INVALID, "group 1 species 4 is not inside");
    memcpy(seg, seg_ok, sizeof seg);
    nets[5].trunk[1].in = 47u;
    EXPECT(mbots_policy_groups_workspace(nets, GROUPS, N, &bytes), MBOTS_E_INVALID, "group 1 species 2: a trunk layer");
    nets[5].trunk[1].in = 48u;

    /* the three calls against the per-net calls on each segment's rows */
    CHECK(mbots_policy_eval_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, out[0], out[1], out[2], ws, bytes,
                                   -1, NULL));
    CHECK(mbots_policy_grad_groups(nets, GROUPS, &seg[0][0], obs, hidden, action, N, g[0], g[1], g[2], grouped, ws,
                                   bytes, -1, NULL));
    for (k = 0; k < 3u; ++k) memset(ref[k], 0, N * sizeof(float));
    for (e = 0; e < SEGS; ++e) {
        const size_t lo = (size_t)seg[e][0], n = (size_t)seg[e][1] - lo;
        uint32_t l;
        if (nets[e].n_trunk == 0) continue;
        CHECK(mbots_policy_grad_workspace(&nets[e], n, &one));
        if (one > bytes) {
            fprintf(stderr, "segment %u: the per-net workspace is larger than the grouped one\n", e);
            return 1;
        }
        CHECK(mbots_policy_eval(&nets[e], obs + lo * 69u, hidden + lo * 16u, action + lo, n, ref[0] + lo, ref[1] + lo,
                                ref[2] + lo, ws, bytes, -1, NULL));
        CHECK(mbots_policy_grad(&nets[e], obs + lo * 69u, hidden + lo * 16u, action + lo, n, g[0] + lo, g[1] + lo,
                                g[2] + lo, &single[e], ws, bytes, -1, NULL));
        for (l = 0; l < nets[e].n_trunk; ++l)
            if (!same_layer(&nets[e].trunk[l], &grouped[e].trunk[l], &single[e].trunk[l], "a trunk layer's gradient", e)) return 1;
        for (l = 0; l < 2u; ++l)
            if (!same_layer(&nets[e].actor[l], &grouped[e].actor[l], &single[e].actor[l], "an actor layer's gradient", e) ||
                !same_layer(&nets[e].critic[l], &grouped[e].critic[l], &single[e].critic[l], "a critic layer's gradient", e))
                return 1;
    }
    for (k = 0; k < 3u; ++k)
        if (!same(out[k], ref[k], N, k == 0 ? "logp" : k == 1 ? "value" : "entropy", 99u)) return 1;
    /* the empty segment's gradients are zeros; the comparison was not one of zeros */
    for (i = 0; i < 48u * 48u; ++i)
        if (grouped[5].actor[0].weight[i] != 0.0f) return 1;
    for (i = 0, k = 0; i < 48u * 48u; ++i) k += grouped[6].actor[0].weight[i] != 0.0f;
    if (k < 48u || out[1][3] == 0.0f || out[0][2] != 0.0f || out[0][210] != 0.0f) {
        fprintf(stderr, "unexpected zeros\n");
        return 1;
    }
    printf("ok rows %u segments %u workspace %llu\n", N, SEGS, (unsigned long long)bytes);
    free(ws);
    return 0;
}
