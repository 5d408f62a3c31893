// The level chain and the workspace of pano_fill_u8 (fill.hip), as plain C++: no device code, so a
// host program can include it alone.  pano360_amd/fill.py states the same arithmetic.
#pragma once
#include <stdint.h>

#include "../../include/pano360.h"

#define FILL_MAX_LEVELS PANO_VIEW_MAX_LEVELS
#define FILL_TEXEL 16               // bytes of a level >= 1's pixel: float32 r, g, b, validity
#define FILL_HEADER 256             // the workspace starts with the "any pixel valid" word

struct FillLayout {
    int n;                          // levels 0 .. n - 1, the last is 1 x 1
    int tail;                       // the first level of at most PANO_FILL_TAIL_PIXELS pixels
    int h[FILL_MAX_LEVELS], w[FILL_MAX_LEVELS];
    int64_t off[FILL_MAX_LEVELS];   // byte offset of level l >= 1 in the workspace (off[0] = 0, unused)
    int64_t bytes;                  // the workspace's size
    int lds[FILL_MAX_LEVELS + 1];   // texel offset of level l >= tail in the tail's LDS; lds[n]: their sum
};

static inline int64_t fill_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// 0 when the sides are outside 1 .. PANO_VIEW_MAX_SIDE, else 1 and the layout
static inline int fill_layout(int h, int w, FillLayout *L) {
    if (h < 1 || w < 1 || h > PANO_VIEW_MAX_SIDE || w > PANO_VIEW_MAX_SIDE) return 0;
    *L = FillLayout();
    L->h[0] = h;
    L->w[0] = w;
    L->n = 1;
    while (L->h[L->n - 1] > 1 || L->w[L->n - 1] > 1) {
        if (L->n == FILL_MAX_LEVELS) return 0;      // (32768 halves to 1 in 15 steps)
        L->h[L->n] = (L->h[L->n - 1] + 1) / 2;
        L->w[L->n] = (L->w[L->n - 1] + 1) / 2;
        ++L->n;
    }
    int64_t at = FILL_HEADER;
    for (int l = 1; l < L->n; ++l) {
        L->off[l] = at;
        at = fill_align(at + (int64_t)FILL_TEXEL * L->h[l] * L->w[l]);
    }
    L->bytes = at;
    L->tail = 0;
    while ((int64_t)L->h[L->tail] * L->w[L->tail] > PANO_FILL_TAIL_PIXELS) ++L->tail;
    int texels = 0;
    for (int l = L->tail; l < L->n; ++l) {
        L->lds[l] = texels;
        texels += L->h[l] * L->w[l];
    }
    L->lds[L->n] = texels;
    return 1;
}
