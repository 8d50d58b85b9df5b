/* A C99 host of the grouped sequence calls of the C ABI (include/mbots.h, "Every
 * group's recurrent nets in one call") on the host path (device == -1): two
 * groups of recurrent nets built from a fixed integer sequence -- different
 * widths and depths, one pair without a net (n_trunk == 0) --, 300 padded
 * sequences of up to 3 steps whose net ids are scattered through the batch
 * (some name no net), and the four calls.  It checks the refusals (a workspace
 * that is too small, a NULL `out`, NULL segments, a net without a memory head,
 * overlapping segments, an order entry out of range, a column named twice, a
 * length outside [0, L], a present action outside 0..5), then prints a digest
 * of order, segments, the four outputs and every gradient, the memory heads'
 * included.  tests/test_policy_seq_groups_c_host.py builds it with gcc -std=c99
 * -pedantic -Werror and compares the digest with
 * madrona_bots.evaluate_sequences_groups + backward(). */
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
#define L 3u
#define B 300u

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
static uint32_t next(uint32_t mod)
{
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 16) % mod;
}
static float *fill(size_t n, float div)
{
    float *p = (float *)malloc((n ? n : 1u) * sizeof(float));
    size_t i;
    if (!p) exit(2);
    for (i = 0; i < n; ++i) p[i] = (float)((int)next(2001u) - 1000) / div;
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
    static struct mbots_policy_net nets[SEGS], bad[SEGS];
    static struct mbots_policy_grads grads[SEGS];
    static int32_t action[L * B], length[B], net_id[B], order[B], order2[B], seg[SEGS][2], seg2[SEGS][2];
    static float logp[L * B], value[L * B], entropy[L * B], hidden[L * B * 16u];
    float *obs, *hidden0, *g[3];
    uint64_t d = 1469598103934665603ull, bytes = 0, small = 0;
    void *ws;
    uint32_t e, i, l, col;
    int32_t keep;

    memset(nets, 0, sizeof nets);
    memset(grads, 0, sizeof grads);
    for (e = 0; e < SEGS; ++e) {
        const uint32_t H = e >= 4u ? 32u : 16u, T = 1u + (e & 1u);
        if (e == 2u) continue;   /* group 0 species 3 has no net */
        nets[e].n_trunk = T;
        nets[e].flags = MBOTS_POLICY_MEMORY_IN;
        for (l = 0; l < T; ++l)
            layer(&nets[e].trunk[l], &grads[e].trunk[l], l ? H : 85u, H, (int32_t)(1u + (e + l) % 5u),
                  l ? 2048.0f : 16384.0f);
        layer(&nets[e].actor[0], &grads[e].actor[0], H, H, 0, 2048.0f);
        layer(&nets[e].actor[1], &grads[e].actor[1], H, 6, 0, 1024.0f);
        layer(&nets[e].critic[0], &grads[e].critic[0], H, H, 0, 2048.0f);
        layer(&nets[e].critic[1], &grads[e].critic[1], H, 1, 0, 2048.0f);
        layer(&nets[e].memory, &grads[e].memory, H, 16u, 0, 512.0f);
    }
    obs = fill((size_t)L * B * 69u, 8.0f);
    hidden0 = fill((size_t)B * 16u, 1000.0f);
    for (i = 0; i < 3u; ++i) g[i] = fill(L * B, 65536.0f);
    for (i = 0; i < L * B; ++i) action[i] = (int32_t)next(6u);
    for (i = 0; i < B; ++i) length[i] = (int32_t)next(L + 1u);
    for (i = 0; i < B; ++i) net_id[i] = (int32_t)next(SEGS + 2u) - 1;   /* -1 and SEGS: no net */

    /* the sort: a stable counting sort, the tail -1 */
    CHECK(mbots_policy_seq_order(net_id, B, GROUPS, order, &seg[0][0], NULL, 0, -1, NULL));
    EXPECT(mbots_policy_seq_order(net_id, B, 65, order2, &seg2[0][0], NULL, 0, -1, NULL), MBOTS_E_INVALID, "groups");
    if (seg[0][0] != 0 || seg[SEGS - 1u][1] >= (int32_t)B || order[B - 1u] != -1) return 1;
    for (e = 0; e < SEGS; ++e) {
        if (e && seg[e][0] != seg[e - 1u][1]) return 1;
        for (i = (uint32_t)seg[e][0]; i < (uint32_t)seg[e][1]; ++i)
            if (net_id[order[i]] != (int32_t)e || (i > (uint32_t)seg[e][0] && order[i] <= order[i - 1u])) return 1;
    }

    CHECK(mbots_policy_seq_groups_workspace(nets, GROUPS, L, B, &bytes));
    ws = malloc((size_t)bytes + 64u);
    if (!ws || !bytes) return 2;
    ws = (void *)(((uintptr_t)ws + 63u) & ~(uintptr_t)63u);

#define EVAL(nets_, order_, seg_, bytes_)                                                                         \
    mbots_policy_seq_eval_groups(nets_, GROUPS, order_, seg_, obs, action, length, hidden0, L, B, logp, value,    \
                                 entropy, hidden, ws, bytes_, -1, NULL)
#define GRAD(out_)                                                                                                \
    mbots_policy_seq_grad_groups(nets, GROUPS, order, &seg[0][0], obs, action, length, hidden0, L, B, g[0], g[1], \
                                 g[2], out_, ws, bytes, -1, NULL)
    /* refusals */
    EXPECT(mbots_policy_seq_groups_workspace(nets, 0, L, B, &small), MBOTS_E_INVALID, "groups");
    EXPECT(EVAL(nets, order, &seg[0][0], bytes - 1u), MBOTS_E_INVALID, "workspace");
    EXPECT(GRAD(NULL), MBOTS_E_INVALID, "null");
    EXPECT(EVAL(nets, order, NULL, bytes), MBOTS_E_INVALID, "segments");
    EXPECT(EVAL(nets, NULL, &seg[0][0], bytes), MBOTS_E_INVALID, "order");
    memcpy(bad, nets, sizeof bad);
    bad[1].memory.weight = NULL;
    EXPECT(mbots_policy_seq_groups_workspace(bad, GROUPS, L, B, &small), MBOTS_E_INVALID,
           "group 0 species 2: sequences are evaluated by a net with a memory head");
    EXPECT(EVAL(bad, order, &seg[0][0], bytes), MBOTS_E_INVALID, "mbots_policy_eval_groups");
    memcpy(seg2, seg, sizeof seg2);
    seg2[4][0] -= 1;   /* into group 0 species 4 */
    EXPECT(EVAL(nets, order, &seg2[0][0], bytes), MBOTS_E_INVALID, "group 0 species 4 and group 1 species 1 overlap");
    memcpy(seg2, seg, sizeof seg2);
    seg2[7][1] = (int32_t)B + 1;
    EXPECT(EVAL(nets, order, &seg2[0][0], bytes), MBOTS_E_INVALID, "group 1 species 4 is not inside");
    memcpy(order2, order, sizeof order2);
    order2[seg[5][0]] = (int32_t)B;
    EXPECT(EVAL(nets, order2, &seg[0][0], bytes), MBOTS_E_INVALID, "group 1 species 2: order[");
    order2[seg[5][0]] = order[seg[0][0]];
    EXPECT(EVAL(nets, order2, &seg[0][0], bytes), MBOTS_E_INVALID, "a second time");
    for (col = 0; col < B && !(net_id[col] == 6 && length[col] == (int32_t)L); ++col) {}
    if (col == B) return 1;
    length[col] = (int32_t)L + 1;
    EXPECT(EVAL(nets, order, &seg[0][0], bytes), MBOTS_E_INVALID, "group 1 species 3: length");
    length[col] = (int32_t)L;
    keep = action[(L - 1u) * B + col];
    action[(L - 1u) * B + col] = 6;
    EXPECT(GRAD(grads), MBOTS_E_INVALID, "group 1 species 3: action 6 of step 2");
    action[(L - 1u) * B + col] = keep;
    /* a column of no net is not looked at */
    for (col = 0; col < B && net_id[col] != -1; ++col) {}
    if (col == B) return 1;
    keep = length[col];
    length[col] = 77;
    CHECK(EVAL(nets, order, &seg[0][0], bytes));
    length[col] = keep;

    CHECK(EVAL(nets, order, &seg[0][0], bytes));
    d = fnv1a(order, sizeof order, d);
    d = fnv1a(seg, sizeof seg, d);
    d = fnv1a(logp, sizeof logp, d);
    d = fnv1a(value, sizeof value, d);
    d = fnv1a(entropy, sizeof entropy, d);
    d = fnv1a(hidden, sizeof hidden, d);
    CHECK(GRAD(grads));
    for (e = 0; e < SEGS; ++e) {
        if (nets[e].n_trunk == 0) continue;
        for (l = 0; l < nets[e].n_trunk; ++l) d = digest_layer(&nets[e].trunk[l], &grads[e].trunk[l], d);
        for (l = 0; l < 2u; ++l) d = digest_layer(&nets[e].actor[l], &grads[e].actor[l], d);
        for (l = 0; l < 2u; ++l) d = digest_layer(&nets[e].critic[l], &grads[e].critic[l], d);
        d = digest_layer(&nets[e].memory, &grads[e].memory, d);
    }
    /* the columns of no net are +0; a memory head received a gradient */
    for (l = 0; l < L; ++l)
        if (logp[l * B + col] != 0.0f || value[l * B + col] != 0.0f || hidden[(l * B + col) * 16u] != 0.0f) return 1;
    for (i = 0; i < 16u * 32u; ++i)
        if (grads[6].memory.weight[i] != 0.0f) break;
    if (i == 16u * 32u) return 1;

    printf("sequences %u digest %016llx\n", B, (unsigned long long)d);
    return 0;
}
