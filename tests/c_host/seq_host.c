/* A C99 host of the trajectory window's sequences and batches (include/mbots.h,
 * "Sequences for a recurrent learner"), in MBOTS_EXEC_CPU mode: it opens a
 * window with every flag, pushes the initial table and one per step under an
 * episode length, computes, numbers the sequences, materialises the whole
 * batch and a gather of a table of its own, chains a second window with
 * keep_last across a capacity growth, checks the refusals and prints a digest
 * of the SEQ_ID / SEQ_POS views, every batch field and the gather of both
 * windows.  tests/test_seq_c_host.py builds it with gcc -std=c99 -pedantic
 * -Werror and compares the digest with the same calls made through
 * madrona_bots. */
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

#define HORIZON 6u
#define MAX_ROWS 256u
#define OBS 69u

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

static float values[MAX_ROWS];
static float own[HORIZON][MAX_ROWS][2];   /* the host's own per-table rows: (table, row) */

static int push(mbots_handle *h, uint32_t step)
{
    uint32_t n = 0, r;
    CHECK(mbots_num_agents(h, &n));
    if (n > MAX_ROWS) {
        fprintf(stderr, "%u rows\n", n);
        return 1;
    }
    for (r = 0; r < n; ++r) values[r] = 0.25f * (float)r - (float)step;
    CHECK(mbots_traj_push(h, values, NULL));
    return 0;
}

/* compute, sequences, the whole batch and a gather, folded into the digest */
static int digest_window(mbots_handle *h, uint64_t *digest, uint64_t *S_out)
{
    int64_t rows[HORIZON];
    uint32_t n = 0, t;
    uint64_t S = 0, LB;
    int32_t what;
    mbots_tensor v;
    struct mbots_traj_batch b;
    const void *tables[HORIZON];
    float *g;
    memset(&b, 0, sizeof(b));
    CHECK(mbots_traj_compute(h, 0.99f, 0.95f, -1.0f, rows, &n, NULL));
    EXPECT(mbots_traj_view(h, MBOTS_TRAJ_SEQ_ID, 0, &v), MBOTS_E_INVALID);    /* not numbered yet */
    EXPECT(mbots_traj_batch(h, 0, 0, &b, NULL), MBOTS_E_INVALID);
    CHECK(mbots_traj_sequences(h, &S, NULL));
    for (t = 0; t < n; ++t)
        for (what = MBOTS_TRAJ_SEQ_ID; what <= MBOTS_TRAJ_SEQ_POS; ++what) {
            CHECK(mbots_traj_view(h, what, t, &v));
            if (v.dims[0] != rows[t] || v.dims[1] != 1 || v.dtype != MBOTS_DTYPE_INT32) return 1;
            *digest = fnv1a(v.data, (size_t)v.dims[0] * 4u, *digest);
        }
    LB = (uint64_t)n * S;
    b.rows = (int32_t *)malloc(LB * 4u);
    b.t0 = (int32_t *)malloc(S * 4u);
    b.len = (int32_t *)malloc(S * 4u);
    b.end = (int32_t *)malloc(S * 4u);
    b.obs = (float *)malloc(LB * OBS * 4u);
    b.reward = (float *)malloc(LB * 4u);
    b.value = (float *)malloc(LB * 4u);
    b.adv = (float *)malloc(LB * 4u);
    b.ret = (float *)malloc(LB * 4u);
    b.action_in = (uint8_t *)malloc(LB);
    b.hidden0 = (float *)malloc(S * 16u * 4u);
    g = (float *)malloc(LB * 8u);
    if (!b.rows || !b.t0 || !b.len || !b.end || !b.obs || !b.reward || !b.value || !b.adv || !b.ret ||
        !b.action_in || !b.hidden0 || !g)
        return 1;
    EXPECT(mbots_traj_batch(h, 0, S + 1u, &b, NULL), MBOTS_E_RANGE);
    EXPECT(mbots_traj_batch(h, 2, 1, &b, NULL), MBOTS_E_RANGE);
    CHECK(mbots_traj_batch(h, 0, S, &b, NULL));
    *digest = fnv1a(b.rows, LB * 4u, *digest);
    *digest = fnv1a(b.t0, S * 4u, *digest);
    *digest = fnv1a(b.len, S * 4u, *digest);
    *digest = fnv1a(b.end, S * 4u, *digest);
    *digest = fnv1a(b.obs, LB * OBS * 4u, *digest);
    *digest = fnv1a(b.reward, LB * 4u, *digest);
    *digest = fnv1a(b.value, LB * 4u, *digest);
    *digest = fnv1a(b.adv, LB * 4u, *digest);
    *digest = fnv1a(b.ret, LB * 4u, *digest);
    *digest = fnv1a(b.action_in, LB, *digest);
    *digest = fnv1a(b.hidden0, S * 16u * 4u, *digest);
    for (t = 0; t < n; ++t) tables[t] = own[t];
    EXPECT(mbots_traj_gather(h, 0, S, tables, n - 1u, 8u, g, NULL), MBOTS_E_INVALID);   /* one per table */
    EXPECT(mbots_traj_gather(h, 0, S, tables, n, 6u, g, NULL), MBOTS_E_INVALID);
    CHECK(mbots_traj_gather(h, 0, S, tables, n, 8u, g, NULL));
    *digest = fnv1a(g, LB * 8u, *digest);
    free(b.rows); free(b.t0); free(b.len); free(b.end); free(b.obs); free(b.reward); free(b.value);
    free(b.adv); free(b.ret); free(b.action_in); free(b.hidden0); free(g);
    *S_out = S;
    return 0;
}

int main(void)
{
    mbots_config cfg;
    mbots_handle *h = NULL;
    struct mbots_traj_batch b;
    uint32_t s, n = 0, t, r;
    uint64_t S1 = 0, S2 = 0, S = 0, digest = 1469598103934665603ull;
    float obs1[OBS];

    for (t = 0; t < HORIZON; ++t)
        for (r = 0; r < MAX_ROWS; ++r) {
            own[t][r][0] = (float)t;
            own[t][r][1] = (float)r;
        }
    memset(&cfg, 0, sizeof(cfg));
    memset(&b, 0, sizeof(b));
    cfg.sensor_size = 32;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    cfg.num_worlds = 4;
    cfg.rand_seed = 15;
    cfg.init_num_agents_per_world = 8;
    cfg.world_offset = 3;
    CHECK(mbots_create(&cfg, &h));
    /* a flagless window refuses the new calls; so does one without the records */
    CHECK(mbots_traj_open(h, HORIZON, MAX_ROWS));
    CHECK(mbots_traj_push(h, NULL, NULL));
    CHECK(mbots_traj_compute(h, 0.99f, 1.0f, 0.0f, NULL, NULL, NULL));
    EXPECT(mbots_traj_sequences(h, &S, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_traj_batch(h, 0, 0, &b, NULL), MBOTS_E_INVALID);
    CHECK(mbots_traj_close(h));
    EXPECT(mbots_traj_open_ex(h, HORIZON, MAX_ROWS, 8u), MBOTS_E_INVALID);
    CHECK(mbots_traj_open_ex(h, HORIZON, MAX_ROWS, MBOTS_TRAJ_SEQ));
    CHECK(mbots_traj_push(h, NULL, NULL));
    EXPECT(mbots_traj_sequences(h, &S, NULL), MBOTS_E_INVALID);          /* no compute yet */
    CHECK(mbots_traj_compute(h, 0.99f, 1.0f, 0.0f, NULL, NULL, NULL));
    CHECK(mbots_traj_sequences(h, &S, NULL));
    if (S != 32u) {
        fprintf(stderr, "%lu sequences in the initial table\n", (unsigned long)S);
        return 1;
    }
    b.obs = obs1;
    EXPECT(mbots_traj_batch(h, 0, 1, &b, NULL), MBOTS_E_INVALID);        /* no MBOTS_TRAJ_REC_OBS */
    b.obs = NULL;
    b.hidden0 = obs1;
    EXPECT(mbots_traj_batch(h, 0, 1, &b, NULL), MBOTS_E_INVALID);        /* no MBOTS_TRAJ_REC_STATE */
    CHECK(mbots_traj_close(h));

    CHECK(mbots_traj_open_ex(h, HORIZON, MAX_ROWS, MBOTS_TRAJ_REC_OBS | MBOTS_TRAJ_REC_STATE));
    CHECK(mbots_set_episode_length(h, 3u));
    if (push(h, 0)) return 1;
    for (s = 0; s < 2u * (HORIZON - 1u); ++s) {
        CHECK(mbots_write_synthetic_actions(h, 1234u, s, 1, NULL));
        CHECK(mbots_step(h, NULL));
        if (push(h, s + 1u)) return 1;
        if (s + 2u == HORIZON) {                /* the first window is full */
            if (digest_window(h, &digest, &S1)) return 1;
            CHECK(mbots_traj_clear(h, 1));
            EXPECT(mbots_traj_sequences(h, &S, NULL), MBOTS_E_INVALID);  /* a clear invalidates */
            CHECK(mbots_grow_capacity(h, 256u)); /* leaves the window intact */
        }
    }
    if (digest_window(h, &digest, &S2)) return 1;
    CHECK(mbots_traj_close(h));
    EXPECT(mbots_traj_sequences(h, &S, NULL), MBOTS_E_INVALID);
    CHECK(mbots_num_agents(h, &n));
    CHECK(mbots_destroy(h));
    printf("agents %u sequences %lu %lu digest %016llx\n", n, (unsigned long)S1, (unsigned long)S2,
           (unsigned long long)digest);
    return 0;
}
