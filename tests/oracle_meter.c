/* tests/oracle_meter.c -- TEST INFRASTRUCTURE ONLY: light metering (include/vrt.h vrt_meter_hdr, points E1-E9) restated in scalar C,
 * written from the header and from nothing of the product's code. tests/oracle_hdr.c, included unchanged, brings h = o_hdr_value, the
 * tone map (o_hdr_tonemap) and the unorm8 store. Every operation rounded on its own (built with oracle/Makefile's flags: no
 * contraction, no fast-math).
 * plant: 0 the rule; 1 the half-bin centre left out of E6; 2 black pixels enter S (and M); 3 the window taken over the non-black
 * pixels instead of all ranks; 4 adapt applied on the first frame; 5 tm->exposure ignored under a record. */
#include "oracle_hdr.c"

#include <string.h>

#define O_METER_BINS 256

typedef struct { float key; int32_t low_permille, high_permille; float min_exposure, max_exposure, adapt; int32_t x0, y0, x1, y1; } o_meter;
typedef struct { float exposure, metered; uint32_t window, frames; } o_exposure;

static uint32_t o_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
static float o_from_bits(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

/* E1 */
float o_meter_luminance(float r, float g, float b) {
    return (0.2126f * o_hdr_value(r) + 0.7152f * o_hdr_value(g)) + 0.0722f * o_hdr_value(b);
}

/* E2 */
int o_meter_bin(float y) {
    const int k = (int)(o_bits(y) >> 20) - 888;
    return k < 0 ? 0 : k;
}

/* E3: the counts of the rectangle [x0, x1) x [y0, y1) of a width x height image (all four 0: the whole frame) */
void o_meter_histogram(const float *rgb, int width, int height, int x0, int y0, int x1, int y1, uint32_t *hist) {
    if (x0 == 0 && y0 == 0 && x1 == 0 && y1 == 0) { x1 = width; y1 = height; }
    for (int k = 0; k < O_METER_BINS; k++) hist[k] = 0;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            const float *c = rgb + ((size_t)y * (size_t)width + (size_t)x) * 3;
            hist[o_meter_bin(o_meter_luminance(c[0], c[1], c[2]))]++;
        }
}

/* E4-E8: hist -> *io. Returns M. */
uint64_t o_meter_resolve(const uint32_t *hist, const o_meter *m, o_exposure *io, int plant) {
    uint64_t n = 0;
    for (int k = plant == 3 ? 1 : 0; k < O_METER_BINS; k++) n += hist[k];
    const uint64_t a = n * (uint64_t)m->low_permille / 1000, b = n * (uint64_t)m->high_permille / 1000;
    uint64_t cum = 0, M = 0, S = 0;
    for (int k = plant == 3 ? 1 : 0; k < O_METER_BINS; k++) {
        const uint64_t lo = cum > a ? cum : a;
        cum += hist[k];
        const uint64_t hi = cum < b ? cum : b;
        const uint64_t nk = hi > lo ? hi - lo : 0;
        if (k == 0 && plant != 2) continue;
        M += nk;
        S += nk * (uint64_t)k;
    }
    float metered = 0.0f, target;
    if (M != 0) {
        const uint64_t t = (S << 20) / M;
        metered = o_from_bits((888u << 20) + (uint32_t)t + (plant == 1 ? 0u : (1u << 19)));
        target = fmin_c(fmax_c(m->key / metered, m->min_exposure), m->max_exposure);
    } else {
        target = io->frames > 0 ? io->exposure : fmin_c(fmax_c(1.0f, m->min_exposure), m->max_exposure);
    }
    float e = target;
    const int first = io->frames == 0 && plant != 4;
    if (!(m->adapt == 1.0f || first || M == 0)) {
        const float prev = io->exposure;
        e = prev + m->adapt * (target - prev);
    }
    io->exposure = e;
    io->metered = metered;
    io->window = (uint32_t)M;
    io->frames = io->frames == 0xffffffffu ? io->frames : io->frames + 1u;
    return M;
}

/* E9: io == NULL: no record */
void o_meter_tonemap(const float *rgb, size_t pixels, int op, float tm_exposure, const o_exposure *io, int plant, uint8_t *rgba8) {
    float e = tm_exposure;
    if (io) e = plant == 5 ? fmin_c(io->exposure, 3.402823466e38f) : fmin_c(tm_exposure * io->exposure, 3.402823466e38f);
    o_hdr_tonemap(rgb, pixels, op, e, rgba8);
}
