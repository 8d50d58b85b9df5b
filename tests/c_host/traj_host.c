/* A C99 host of the trajectory window of the C ABI (include/mbots.h,
 * "Trajectory window"), in MBOTS_EXEC_CPU mode: it opens a window, pushes the
 * initial table and one per step with values of its own under an episode
 * length (so lifelines are cut by resets too), computes, chains a second
 * window with keep_last, grows the capacity in between, checks the refusals
 * (a full window, a table outside it, every call after the close) and prints
 * a digest of all eight views of both windows.
 * tests/test_traj_c_host.py builds it with gcc -std=c99 -pedantic -Werror and
 * compares the digest with the same calls made through madrona_bots;
 * scripts/asan_host.sh runs it against a sanitised CPU-mode library. */
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

/* push the current table with values 0.25 * row - step */
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

/* compute, then fold every view of every table into the digest */
static int digest_window(mbots_handle *h, uint64_t *digest)
{
    int64_t rows[HORIZON];
    uint32_t n = 0, t;
    int32_t what;
    mbots_tensor v;
    CHECK(mbots_traj_compute(h, 0.99f, 0.95f, -1.0f, rows, &n, NULL));
    for (t = 0; t < n; ++t)
        for (what = MBOTS_TRAJ_LINK; what <= MBOTS_TRAJ_RET; ++what) {
            if (what == MBOTS_TRAJ_NEXT && t + 1 == n) {
                EXPECT(mbots_traj_view(h, what, t, &v), MBOTS_E_RANGE);
                continue;
            }
            CHECK(mbots_traj_view(h, what, t, &v));
            if (v.dims[0] != rows[t] || v.dims[1] != 1 || v.device != -1) {
                fprintf(stderr, "view %d of table %u: %ld x %ld\n", what, t, (long)v.dims[0], (long)v.dims[1]);
                return 1;
            }
            *digest = fnv1a(v.data, (size_t)v.dims[0] * 4u, *digest);
        }
    EXPECT(mbots_traj_view(h, MBOTS_TRAJ_LINK, n, &v), MBOTS_E_RANGE);
    return 0;
}

int main(void)
{
    mbots_config cfg;
    mbots_handle *h = NULL;
    mbots_tensor v;
    uint32_t s, n = 0, info[4];
    uint64_t digest = 1469598103934665603ull;

    memset(&cfg, 0, sizeof(cfg));
    cfg.sensor_size = 32;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    cfg.num_worlds = 4;
    cfg.rand_seed = 15;
    cfg.init_num_agents_per_world = 8;
    cfg.world_offset = 3;
    CHECK(mbots_create(&cfg, &h));
    EXPECT(mbots_traj_push(h, NULL, NULL), MBOTS_E_INVALID);           /* no window yet */
    EXPECT(mbots_traj_open(h, 1, MAX_ROWS), MBOTS_E_INVALID);
    CHECK(mbots_traj_open(h, HORIZON, MAX_ROWS));
    EXPECT(mbots_traj_open(h, HORIZON, MAX_ROWS), MBOTS_E_INVALID);    /* one per manager */
    CHECK(mbots_schedule_info(h, info));
    if (info[0] & 32u) {
        fprintf(stderr, "a window armed the manager\n");
        return 1;
    }
    CHECK(mbots_set_episode_length(h, 3u));
    if (push(h, 0)) return 1;
    for (s = 0; s < 2u * (HORIZON - 1u); ++s) {
        CHECK(mbots_write_synthetic_actions(h, 1234u, s, 0, NULL));
        CHECK(mbots_step(h, NULL));
        if (push(h, s + 1u)) return 1;
        if (s + 2u == HORIZON) {                /* the first window is full */
            EXPECT(mbots_traj_push(h, NULL, NULL), MBOTS_E_INVALID);
            if (digest_window(h, &digest)) return 1;
            CHECK(mbots_traj_clear(h, 1));
            CHECK(mbots_traj_num_tables(h, &n));
            if (n != 1u) {
                fprintf(stderr, "%u tables after clear(keep_last)\n", n);
                return 1;
            }
            CHECK(mbots_grow_capacity(h, 256u)); /* leaves the window intact */
        }
    }
    if (digest_window(h, &digest)) return 1;
    CHECK(mbots_traj_clear(h, 0));
    CHECK(mbots_traj_num_tables(h, &n));
    EXPECT(mbots_traj_compute(h, 0.99f, 1.0f, 0.0f, NULL, NULL, NULL), MBOTS_E_INVALID);   /* empty */
    CHECK(mbots_traj_close(h));
    EXPECT(mbots_traj_view(h, MBOTS_TRAJ_LINK, 0, &v), MBOTS_E_INVALID);
    EXPECT(mbots_traj_clear(h, 0), MBOTS_E_INVALID);
    EXPECT(mbots_traj_close(h), MBOTS_E_INVALID);
    CHECK(mbots_traj_open(h, 2, 1));            /* left open: mbots_destroy frees it */
    CHECK(mbots_num_agents(h, &n));
    CHECK(mbots_destroy(h));
    printf("agents %u digest %016llx\n", n, (unsigned long long)digest);
    return 0;
}
