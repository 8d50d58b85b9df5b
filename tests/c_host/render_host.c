/* A C99 host of the rasteriser of the C ABI (include/mbots.h, "Rasteriser"), in
 * MBOTS_EXEC_CPU mode: it steps a 3-world manager, renders worlds 0 and 1 with
 * the NULL-list form (k = 2 < num_worlds), checks that an explicit list gives
 * the same bytes (reversed: the images swapped), that the palette call agrees
 * with the rgb of the class map, and the status codes -- every refusal leaving
 * the outputs as they were -- and prints a digest of the three outputs.
 * tests/test_render_c_host.py builds it with gcc -std=c99 -pedantic -Werror and
 * compares the digest with the same render through madrona_bots. */
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

#define SCALE 4u
#define K 2u
#define PIX ((size_t)(96u * SCALE) * (128u * SCALE))

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

int main(void)
{
    mbots_config cfg;
    mbots_handle *h = NULL;
    mbots_render_out out, none, part;
    uint8_t pal[36], *cls, *rgb, *cls2, *rgb2;
    int16_t *slot, *slot2;
    uint32_t s, list[3];
    uint64_t digest = 1469598103934665603ull;
    size_t i;

    memset(&cfg, 0, sizeof(cfg));
    cfg.sensor_size = 32;
    cfg.exec_mode = MBOTS_EXEC_CPU;
    cfg.num_worlds = 3;
    cfg.rand_seed = 15;
    cfg.init_num_agents_per_world = 24;
    cfg.flags = MBOTS_FLAG_SHARD_GHOST;
    CHECK(mbots_create(&cfg, &h));
    for (s = 0; s < 6u; ++s) {
        CHECK(mbots_write_synthetic_actions(h, 1234u, s, 1, NULL));
        CHECK(mbots_step(h, NULL));
    }
    cls = (uint8_t *)malloc(K * PIX);
    slot = (int16_t *)malloc(K * PIX * sizeof(int16_t));
    rgb = (uint8_t *)malloc(K * PIX * 3u);
    cls2 = (uint8_t *)malloc(K * PIX);
    slot2 = (int16_t *)malloc(K * PIX * sizeof(int16_t));
    rgb2 = (uint8_t *)malloc(K * PIX * 3u);
    if (!cls || !slot || !rgb || !cls2 || !slot2 || !rgb2) return 1;
    out.cls = cls;
    out.slot = slot;
    out.rgb = rgb;
    CHECK(mbots_render_worlds(h, NULL, K, SCALE, &out, NULL));   /* worlds 0 and 1 */

    /* the refusals leave the outputs as they are */
    memcpy(cls2, cls, K * PIX);
    memcpy(slot2, slot, K * PIX * sizeof(int16_t));
    memcpy(rgb2, rgb, K * PIX * 3u);
    none.cls = NULL;
    none.slot = NULL;
    none.rgb = NULL;
    list[0] = 1u;
    list[1] = 3u;                               /* the shard ghost's index: never rendered */
    EXPECT(mbots_render_worlds(h, NULL, K, 3u, &out, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_render_worlds(h, NULL, K, 16u, &out, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_render_worlds(h, NULL, K, SCALE, &none, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_render_worlds(h, NULL, K, SCALE, NULL, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_render_worlds(NULL, NULL, K, SCALE, &out, NULL), MBOTS_E_INVALID);
    EXPECT(mbots_render_worlds(h, list, K, SCALE, &out, NULL), MBOTS_E_RANGE);
    EXPECT(mbots_render_worlds(h, NULL, 4u, SCALE, &out, NULL), MBOTS_E_RANGE);
    EXPECT(mbots_render_worlds(h, list, 0u, SCALE, &out, NULL), MBOTS_OK);
    EXPECT(mbots_render_palette(NULL), MBOTS_E_INVALID);
    if (memcmp(cls2, cls, K * PIX) || memcmp(slot2, slot, K * PIX * sizeof(int16_t)) ||
        memcmp(rgb2, rgb, K * PIX * 3u)) {
        fprintf(stderr, "a refused call wrote its outputs\n");
        return 1;
    }

    /* an explicit list, reversed, one output only: the images swapped */
    list[0] = 1u;
    list[1] = 0u;
    part.cls = cls2;
    part.slot = NULL;
    part.rgb = NULL;
    CHECK(mbots_render_worlds(h, list, K, SCALE, &part, NULL));
    if (memcmp(cls2, cls + PIX, PIX) || memcmp(cls2 + PIX, cls, PIX)) {
        fprintf(stderr, "the listed render differs from the NULL-list render\n");
        return 1;
    }

    /* the palette: rgb of every pixel that is no body is its class's entry */
    CHECK(mbots_render_palette(pal));
    for (i = 0; i < K * PIX; ++i) {
        const unsigned c = cls[i];
        if (c >= 12u || c == 3u || (slot[i] < 0) != (c < (unsigned)MBOTS_RENDER_BODY)) {
            fprintf(stderr, "pixel %lu: class %u, slot %d\n", (unsigned long)i, c, (int)slot[i]);
            return 1;
        }
        if ((c < (unsigned)MBOTS_RENDER_BODY || c >= (unsigned)MBOTS_RENDER_MARK) && memcmp(rgb + 3u * i, pal + 3u * c, 3u)) {
            fprintf(stderr, "pixel %lu: rgb is not the palette's\n", (unsigned long)i);
            return 1;
        }
    }
    digest = fnv1a(cls, K * PIX, digest);
    digest = fnv1a(slot, K * PIX * sizeof(int16_t), digest);
    digest = fnv1a(rgb, K * PIX * 3u, digest);
    digest = fnv1a(pal, sizeof(pal), digest);
    CHECK(mbots_destroy(h));
    free(cls);
    free(slot);
    free(rgb);
    free(cls2);
    free(slot2);
    free(rgb2);
    printf("digest %016llx\n", (unsigned long long)digest);
    return 0;
}
