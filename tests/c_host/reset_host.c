/* A C99 host of the episode entry points of the C ABI (include/mbots.h,
 * "Episodes and resets"), in MBOTS_EXEC_CPU mode: it sets an episode length,
 * drives the identity-keyed action stream, flags worlds through
 * mbots_reset_worlds (next episode, explicit episodes, indices of another
 * rank) and through the live MBOTS_EXPORT_RESET view, and prints a digest of
 * the three episode exports and the table's views.
 * tests/test_reset_c_host.py builds it with gcc -std=c99 -pedantic -Werror
 * and compares the digest with the same calls made through madrona_bots. */
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

static size_t elem_size(int32_t dtype)
{
    return dtype == MBOTS_DTYPE_UINT8 || dtype == MBOTS_DTYPE_INT8 ? 1u : 4u;
}

int main(int argc, char **argv)
{
    const uint32_t worlds = argc > 1 ? (uint32_t)atoi(argv[1]) : 6u;
    const uint32_t steps = argc > 2 ? (uint32_t)atoi(argv[2]) : 12u;
    static const int32_t ids[] = {MBOTS_EXPORT_RESET, MBOTS_EXPORT_EPISODE, MBOTS_EXPORT_EPISODE_STEP,
                                  MBOTS_EXPORT_ACTION, MBOTS_EXPORT_REWARD, MBOTS_EXPORT_POSITION,
                                  MBOTS_EXPORT_PREV_POSITION, MBOTS_EXPORT_HEALTH,
                                  MBOTS_EXPORT_SENSOR_SEMANTIC, MBOTS_EXPORT_PREV_SENSOR_SEMANTIC,
                                  MBOTS_EXPORT_STATS, MBOTS_EXPORT_SPECIES_COUNT};
    const uint32_t next[2] = {1u, 1000u};      /* 1000: another rank's, ignored */
    const uint32_t which[2] = {0u, 2u}, eps[2] = {5u, 0u};
    const uint32_t bad = 0x7FFFFFFEu;
    mbots_config cfg;
    mbots_handle *h = NULL;
    mbots_tensor t;
    uint32_t info[4], n = 0, s, k;
    uint64_t digest = 1469598103934665603ull;

    memset(&cfg, 0, sizeof(cfg));
    cfg.sensor_size = 32;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    cfg.num_worlds = worlds;
    cfg.rand_seed = 69;
    cfg.init_num_agents_per_world = 32;
    cfg.world_offset = 1;
    CHECK(mbots_create(&cfg, &h));
    /* an empty list is a no-op and arms nothing; an episode past the bound is refused */
    CHECK(mbots_reset_worlds(h, NULL, 0, NULL, NULL));
    CHECK(mbots_schedule_info(h, info));
    if (info[0] & 32u) {
        fprintf(stderr, "an empty list armed the manager\n");
        return 1;
    }
    if (mbots_reset_worlds(h, which, 1, &bad, NULL) != MBOTS_E_INVALID || mbots_last_error()[0] == '\0') {
        fprintf(stderr, "episode 2^31 - 2 accepted\n");
        return 1;
    }
    CHECK(mbots_set_episode_length(h, 5u));
    CHECK(mbots_schedule_info(h, info));
    if (!(info[0] & 32u)) {
        fprintf(stderr, "an episode length did not arm the manager\n");
        return 1;
    }
    for (s = 0; s < steps; ++s) {
        if (s == 2) CHECK(mbots_reset_worlds(h, next, 2, NULL, NULL));          /* global world 1: local 0 */
        if (s == 4) CHECK(mbots_reset_worlds(h, which, 2, eps, NULL));          /* global 0 is not ours; 2: local 1 */
        if (s == 7) {   /* the live flag view: local world 3 to episode 9 */
            CHECK(mbots_export(h, MBOTS_EXPORT_RESET, &t));
            if (t.dims[0] != (int64_t)worlds || t.dims[1] != 1 || t.dtype != MBOTS_DTYPE_INT32) {
                fprintf(stderr, "reset view: %ld x %ld\n", (long)t.dims[0], (long)t.dims[1]);
                return 1;
            }
            ((int32_t *)t.data)[3] = 9 + 2;
        }
        CHECK(mbots_step(h, NULL));
        CHECK(mbots_shift_observations(h, NULL));
        CHECK(mbots_write_synthetic_actions(h, 1234u, s, 1, NULL));
    }
    CHECK(mbots_num_agents(h, &n));
    for (k = 0; k < sizeof(ids) / sizeof(ids[0]); ++k) {
        CHECK(mbots_export(h, ids[k], &t));
        if (t.device != -1) {
            fprintf(stderr, "export %d: device %d in CPU mode\n", ids[k], t.device);
            return 1;
        }
        digest = fnv1a(t.data, (size_t)(t.dims[0] * t.dims[1]) * elem_size(t.dtype), digest);
    }
    CHECK(mbots_destroy(h));
    printf("agents %u digest %016llx\n", n, (unsigned long long)digest);
    return 0;
}
