// mbots_render.hpp -- the top-down rasteriser's per-(pixel, object) predicates
// (mbots_render_worlds; the spec is include/mbots.h "Rasteriser"), shared by
// render_kernel and the CPU mode so that both give the same bits.  Every
// product and sum is one f32 rounding in the order written
// (-ffp-contract=off); the only division and square root are heading()'s.
#pragma once

#include "mbots_ray.hpp"

namespace mbots {

constexpr int kRenderW = 128, kRenderH = 96;   // image size at scale 1 (one pixel per cell)
constexpr uint32_t kRenderNoSlot = 0xFFFFu;    // a pixel's code without an agent (slot -1 as int16)

// the caller's three optional outputs (mbots_render_out), device or host memory
struct RenderOut {
    uint8_t *cls;
    int16_t *slot;
    uint8_t *rgb;
};

MB_HD bool render_scale_ok(uint32_t s) { return s == 1u || s == 2u || s == 4u || s == 8u; }

// the arena coordinate pixel index i samples: (i + 0.5) / s, exact in f32
MB_HD float render_sample(uint32_t i, float inv_scale) { return ((float)i + 0.5f) * inv_scale; }

// A staged agent: position, heading and what a hit needs of it -- its slot
// (bits 0..15), species - 1 (16..17) and its body's shade k (20..27).
struct RenderAgent {
    float x, y, hx, hy;
    uint32_t info;
};

MB_HD RenderAgent render_agent(uint32_t slot, float x, float y, float rw, float rz, int32_t species, int32_t health)
{
    RenderAgent a;
    a.x = x;
    a.y = y;
    heading(rw, rz, a.hx, a.hy);
    a.info = slot | (((uint32_t)(species - 1) & 3u) << 16) | (render_shade(health) << 20);
    return a;
}

// dy2 = dy * dy of the pixel's row (the same rounding for every pixel of it)
MB_HD bool render_disc_hit(float dx, float dy2) { return dx * dx + dy2 <= kAgentR2; }

// the heading mark inside a disc: ahead of the centre along the heading, narrow across it
MB_HD bool render_mark_hit(float dx, float dy, float hx, float hy)
{
    const float fa = dx * hx + dy * hy, la = dy * hx - dx * hy;
    return (fa >= 0.3f) & (fabsf(la) <= 0.25f);
}

// a hit's pixel code: slot | class << 16 | shade << 20
MB_HD uint32_t render_agent_code(const RenderAgent &a, float dx, float dy)
{
    const uint32_t sp1 = (a.info >> 16) & 3u;
    const uint32_t cls = (render_mark_hit(dx, dy, a.hx, a.hy) ? kClsMark : kClsBody) + sp1;
    return (a.info & 0xFFFFu) | (cls << 16) | (a.info & 0x0FF00000u);
}

// the +-1 food square at (X, Y) rotated by (c, s) = food_cs(rotation)
MB_HD bool render_food_hit(float px, float py, float X, float Y, float c, float s)
{
    const float dx = px - X, dy = py - Y;
    const float u = fabsf(dx * c + dy * s), v = fabsf(dy * c - dx * s);
    return (u <= 1.0f) & (v <= 1.0f);
}

// Conservative culls in y for a band of sample rows [ylo, yhi]: a disc reaches
// no row farther than kAgentR = 0.92 from its centre, a food square none
// farther than its half diagonal sqrt(2) (1.4143 with the polynomial's
// |c^2 + s^2 - 1| < 1e-6); the margins 1 and 1.5 leave 0.08 for the roundings
// of these differences (below 2^-16 in this arena).
constexpr float kRenderAgentReach = 1.0f, kRenderFoodReach = 1.5f;
MB_HD bool render_reaches(float y, float ylo, float yhi, float reach)
{
    return (y >= ylo - reach) & (y <= yhi + reach);
}

// a pixel without an agent: food, else wall, else floor (nf packages: X, Y, c, s)
MB_HD uint32_t render_ground(float px, float py, const float4 *food, int nf)
{
    bool hit = false;
    for (int k = 0; k < nf; ++k) hit |= render_food_hit(px, py, food[k].x, food[k].y, food[k].z, food[k].w);
    return hit ? kClsFood : in_wall_box(px, py) ? kClsWall : kClsFloor;
}

// class and shade of a pixel code
MB_HD uint32_t render_code_cls(uint32_t code) { return (code >> 16) & 15u; }
MB_HD uint32_t render_code_rgb(uint32_t code) { return render_rgb(render_code_cls(code), (code >> 20) & 255u); }

}  // namespace mbots
