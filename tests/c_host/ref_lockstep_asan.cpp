// Stand-alone sanitizer run (scripts/asan_host.sh; never loaded into Python):
// 4 worlds, 20 steps of the oracle (oracle/mbots_oracle.c) in lock-step with the
// reference's simulation code on the stand-in engine (oracle/refbuild/), all
// three built with -fsanitize=address,undefined.  Every exported column must be
// equal after each step and shift, and the sanitizers must stay silent -- in
// particular the reference's read of rewards[4] has to land inside
// the stand-in's own storage, its padding row for the last world.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mbots_oracle.h"

extern "C" {
void *ref_create(uint32_t worlds, uint32_t seed, uint32_t init_agents, uint32_t max_rows);
void ref_destroy(void *h);
void ref_step(void *h);
void ref_sensor(void *h);
void ref_shift_observations(void *h);
uint32_t ref_num_agents(void *h);
int ref_read_column(void *h, int col, int is_prev, void *out);
int ref_write_column(void *h, int col, const void *in, uint32_t rows);
void ref_world_counts(void *h, int32_t *counts, int32_t *offsets);
int32_t ref_world_state(void *h, uint32_t w, float *xy, float *rot, int32_t *species, int32_t *health);
int32_t ref_world_food(void *h, uint32_t w, int32_t *out);
int ref_set_finder(void *h, uint32_t w, const int32_t *slots, uint32_t n);
}

static const size_t kRowBytes[ORC_NUM_COLS] = {4, 8, 4, 8, 4, 24, 16, 64, 32, 32};
static const char *kNames[ORC_NUM_COLS] = {"species", "pos", "health", "surround", "reward",
                                           "action", "stats", "hidden", "semantic", "depth"};

static int compare(orc_sim *orc, void *ref, const char *where, int t)
{
    uint32_t n = orc_num_agents(orc);
    if (ref_num_agents(ref) != n) {
        printf("%s %d: %u reference rows, %u oracle rows\n", where, t, ref_num_agents(ref), n);
        return 1;
    }
    std::vector<char> buf;
    for (int prev = 0; prev < 2; ++prev)
        for (int c = 0; c < ORC_NUM_COLS; ++c) {
            buf.assign(kRowBytes[c] * n + 1, 0);
            ref_read_column(ref, c, prev, buf.data());
            if (memcmp(buf.data(), orc_column(orc, c, prev), kRowBytes[c] * n) != 0) {
                printf("%s %d: column %s%s differs\n", where, t, prev ? "prev_" : "", kNames[c]);
                return 1;
            }
        }
    return 0;
}

int main()
{
    const uint32_t W = 4, A = 32, cap = 256, steps = 20;
    orc_config cfg = {W, 0, 69, A, cap, 0, 1};
    orc_sim *orc = orc_create(&cfg);
    void *ref = ref_create(W, 69, A, 4096);
    if (!orc || !ref) return 2;
    std::vector<int32_t> finder(cap), food(4 * 240), food2(4 * 240);
    int rc = compare(orc, ref, "init", 0);
    for (uint32_t t = 0; t < steps && !rc; ++t) {
        for (uint32_t w = 0; w < W; ++w) {
            int32_t n = 0;
            orc_world_state(orc, w, nullptr, nullptr, nullptr, nullptr, finder.data(), &n);
            if (ref_set_finder(ref, w, finder.data(), (uint32_t)n)) { printf("finder: world %u\n", w); rc = 1; }
        }
        orc_write_synthetic_actions(orc, 1234, t, 1);
        uint32_t n = orc_num_agents(orc);
        ref_write_column(ref, ORC_COL_ACTION, orc_column(orc, ORC_COL_ACTION, 0), n);
        ref_write_column(ref, ORC_COL_HIDDEN, orc_column(orc, ORC_COL_HIDDEN, 0), n);
        orc_step(orc);
        ref_step(ref);
        ref_sensor(ref);
        n = orc_num_agents(orc);
        ref_write_column(ref, ORC_COL_SEMANTIC, orc_column(orc, ORC_COL_SEMANTIC, 0), n);
        ref_write_column(ref, ORC_COL_DEPTH, orc_column(orc, ORC_COL_DEPTH, 0), n);
        if (!rc) rc = compare(orc, ref, "step", (int)t);
        for (uint32_t w = 0; w < W && !rc; ++w) {
            int32_t k = orc_world_food(orc, w, food.data()), k2 = ref_world_food(ref, w, food2.data());
            if (k != k2 || memcmp(food.data(), food2.data(), 16 * (size_t)(k > 0 ? k : 0)) != 0) {
                printf("step %u: world %u food differs (%d / %d packages)\n", t, w, k2, k);
                rc = 1;
            }
        }
        orc_shift_observations(orc);
        ref_shift_observations(ref);
        if (!rc) rc = compare(orc, ref, "shift", (int)t);
    }
    if (orc_overflow(orc)) { printf("the oracle's cap bound\n"); rc = 1; }
    printf("ref_lockstep_asan: %u agents after %u steps, %s\n", orc_num_agents(orc), steps, rc ? "MISMATCH" : "equal");
    orc_destroy(orc);
    ref_destroy(ref);
    return rc;
}
