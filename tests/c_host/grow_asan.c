/* Host AddressSanitizer check (scripts/asan_host.sh; CPU mode, no GPU) of the
 * capacity growth in place: mbots_grow_capacity through capacities that are
 * and are not multiples of 4, with and without the shard ghost, views taken
 * before a growth read after it (the retired lists) and after a step,
 * mbots_release_retired, the refusals, and mbots_set_auto_capacity from 96
 * slots.  Each grown manager must save the checkpoint bytes of a fresh manager
 * of that capacity that loaded its checkpoint, before and after more steps. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mbots.h"
#define CHECK(c) do { int r_ = (c); if (r_ < 0) { fprintf(stderr, "%s: %d %s\n", #c, r_, mbots_last_error()); return 1; } } while (0)
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static int run(mbots_handle *h, int from, int to) {
    for (int t = from; t < to; ++t) {
        CHECK(mbots_write_synthetic_actions(h, 1234, t, 1, NULL));
        int rc = mbots_step(h, NULL); if (rc < 0) { fprintf(stderr, "step %d %s\n", rc, mbots_last_error()); return 1; }
        CHECK(mbots_shift_observations(h, NULL));
    }
    return 0;
}
static int save(mbots_handle *h, void **blob, uint64_t *n) {
    CHECK(mbots_checkpoint_size(h, n));
    *blob = malloc(*n);
    CHECK(mbots_save_checkpoint(h, *blob, *n));
    return 0;
}
/* 1 when both managers save the same bytes */
static int same(mbots_handle *a, mbots_handle *b) {
    void *x = NULL, *y = NULL; uint64_t n = 0, m = 0;
    if (save(a, &x, &n) || save(b, &y, &m)) return 0;
    int eq = n == m && memcmp(x, y, n) == 0;
    free(x); free(y);
    return eq;
}
static int grow_case(uint32_t flags, unsigned cap0, const unsigned *caps, int ncaps) {
    mbots_config c; memset(&c, 0, sizeof c);
    c.num_worlds = 5; c.rand_seed = 69; c.init_num_agents_per_world = 8; c.sensor_size = 32;
    c.agent_capacity = cap0; c.flags = flags; c.exec_mode = MBOTS_EXEC_CPU;
    mbots_handle *a = NULL; CHECK(mbots_create(&c, &a));
    int t = 0;
    if (run(a, t, t + 5)) return 1;
    t += 5;
    for (int i = 0; i < ncaps; ++i) {
        void *blob = NULL; uint64_t n = 0;
        if (save(a, &blob, &n)) return 1;
        mbots_tensor pos; CHECK(mbots_export(a, MBOTS_EXPORT_POSITION, &pos));
        size_t bytes = (size_t)pos.dims[0] * 2 * sizeof(float);
        void *before = malloc(bytes); memcpy(before, pos.data, bytes);
        CHECK(mbots_grow_capacity(a, caps[i]));
        uint32_t cap = 0; CHECK(mbots_capacity(a, &cap)); EXPECT(cap == caps[i]);
        mbots_config d = c; d.agent_capacity = caps[i];
        mbots_handle *b = NULL; CHECK(mbots_create(&d, &b));
        CHECK(mbots_load_checkpoint(b, blob, n));
        EXPECT(same(a, b));
        if (run(a, t, t + 4) || run(b, t, t + 4)) return 1;
        t += 4;
        EXPECT(same(a, b));
        EXPECT(memcmp(before, pos.data, bytes) == 0);   /* the retired storage, after more steps */
        mbots_tensor now; CHECK(mbots_export(a, MBOTS_EXPORT_POSITION, &now)); EXPECT(now.data != pos.data);
        if (i == 0) CHECK(mbots_release_retired(a));   /* (pos dangles from here on) */
        free(before); free(blob); mbots_destroy(b);
    }
    /* refusals leave the manager as it is */
    uint32_t cap = 0; CHECK(mbots_capacity(a, &cap));
    EXPECT(mbots_grow_capacity(a, cap - 1) == MBOTS_E_INVALID);
    EXPECT(mbots_grow_capacity(a, MBOTS_MAX_CAPACITY + 1) == MBOTS_E_INVALID);
    EXPECT(mbots_grow_capacity(a, cap) == MBOTS_OK);
    uint32_t still = 0; CHECK(mbots_capacity(a, &still)); EXPECT(still == cap);
    if (run(a, t, t + 2)) return 1;
    mbots_destroy(a);   /* (with retired storage still held) */
    return 0;
}
static int auto_case(uint32_t flags) {
    mbots_config c; memset(&c, 0, sizeof c);
    c.num_worlds = 6; c.rand_seed = 69; c.init_num_agents_per_world = 32; c.sensor_size = 32;
    c.agent_capacity = 96; c.flags = flags; c.exec_mode = MBOTS_EXEC_CPU;
    mbots_handle *a = NULL, *b = NULL; CHECK(mbots_create(&c, &a));
    mbots_config d = c; d.agent_capacity = 1024; CHECK(mbots_create(&d, &b));
    CHECK(mbots_set_auto_capacity(a, 1));
    if (run(a, 0, 12) || run(b, 0, 12)) return 1;
    uint32_t cap = 0, na = 0, nb = 0; CHECK(mbots_capacity(a, &cap)); EXPECT(cap == 128);
    CHECK(mbots_num_agents(a, &na)); CHECK(mbots_num_agents(b, &nb)); EXPECT(na == nb);
    uint64_t dropped = 1; CHECK(mbots_overflow(a, &dropped)); EXPECT(dropped == 0);
    mbots_destroy(a); mbots_destroy(b);
    return 0;
}
int main(void) {
    const unsigned odd[3] = {77, 128, 513}, classes[2] = {256, 4096};
    if (grow_case(0, 30, odd, 3)) return 1;
    if (grow_case(MBOTS_FLAG_SHARD_GHOST, 128, classes, 2)) return 1;
    if (auto_case(0) || auto_case(MBOTS_FLAG_SHARD_GHOST)) return 1;
    puts("ok");
    return 0;
}
