/* previous_twin.h — TEST ONLY: plain-C99 restatement of the previous-frame rule of DESIGN.md §4 item 18 (gv_device_math.hpp; kernels:
 * gv_previous.hip), the check gv_pool_emit_previous is compared against bit for bit. Compile with -ffp-contract=off: every fused
 * multiply-add is written as fmaf. The product is instance_twin.h's, literally.
 *
 * THE PREVIOUS RULE (the same text stands in DESIGN.md §4 item 18, include/garden_vis.h and gv_device_math.hpp). For draw k of a
 * view: slot s_k, record model M_k, VP = the view's view_proj, the pool's history H (per slot 12 floats and a stamp; an epoch e, 0 =
 * empty; a coverage H.slots; the kept view's view_proj KVP and camera position KC), PVP = prev_view_proj, or KVP when it is NULL,
 * d_r = view.camera_position[r] - KC[r] (one fp32 subtraction per component, done on the host).
 *  1. Cut: GV_PREVIOUS_CUT, or e == 0: every draw is fresh, with PVP = VP and d = (0, 0, 0).
 *  2. Kept <=> no cut && s_k < H.slots && stamp[s_k] == e: P_k = the row's 12 floats.
 *  3. Fresh otherwise: the draw is taken as static in the world. P_k = M_k with c3[r] = M_k.c3[r] + d_r (one fp32 add per component);
 *     the other nine floats verbatim.
 *  4. prev_mvp_k = PVP * P_k exactly as item 9: element i of column j = fma(PVP[12 + i], b3, fma(PVP[8 + i], b2, fma(PVP[4 + i], b1,
 *     fma(PVP[i], b0, +0)))) with (b0, b1, b2) = column j of P_k and b3 = 0, or 1 for j = 3. has_history_k = 1 when kept, 0 when fresh.
 */
#ifndef GV_PREVIOUS_TWIN_H
#define GV_PREVIOUS_TWIN_H
#include <string.h>

#include "instance_twin.h"

/* The history as the twin holds it: rows[16 * s] = the 12 floats of slot s, word 12 the stamp (as the device row), words 13-15 zero. */
typedef struct PreviousTwinHistory {
    uint32_t* rows;            /* [16 * slots] words */
    uint32_t slots;            /* H.slots */
    uint32_t epoch;            /* e */
    float view_proj[16];       /* KVP */
    float camera_position[3];  /* KC */
} PreviousTwinHistory;

/* gv_pool_keep_models over n delivered records: add == 0 advances e (a wrap to 0 clears every stamp and gives 1) and keeps the view.
 * The caller has grown rows to cover every slot of the records, new rows zero. */
static inline void previous_twin_keep(PreviousTwinHistory* h, const float view_proj[16], const float camera_position[3], const uint32_t* slots,
                                      const float* models, uint32_t n, int add)
{
    uint32_t k, s;
    if (!add) {
        if (h->epoch == 0xFFFFFFFFu) {
            for (s = 0; s < h->slots; s++)
                h->rows[16 * (size_t)s + 12] = 0;
            h->epoch = 0;
        }
        h->epoch++;
        memcpy(h->view_proj, view_proj, sizeof(h->view_proj));
        memcpy(h->camera_position, camera_position, sizeof(h->camera_position));
    }
    for (k = 0; k < n; k++) {
        if (slots[k] >= h->slots)
            continue;
        memcpy(h->rows + 16 * (size_t)slots[k], models + 12 * (size_t)k, 48);
        h->rows[16 * (size_t)slots[k] + 12] = h->epoch;
        h->rows[16 * (size_t)slots[k] + 13] = h->rows[16 * (size_t)slots[k] + 14] = h->rows[16 * (size_t)slots[k] + 15] = 0;
    }
}

/* gv_pool_forget_models: count == 0 empties the history */
static inline void previous_twin_forget(PreviousTwinHistory* h, uint32_t first, uint32_t count)
{
    uint64_t s;
    if (count == 0) {
        h->epoch = 0;
        h->slots = 0;
        return;
    }
    for (s = first; s < (uint64_t)first + count && s < h->slots; s++)
        h->rows[16 * (size_t)s + 12] = 0;
}

/* One draw: steps 1 - 4. view_proj / camera_position: the view's own; prev_view_proj may be NULL. Returns has_history. */
static inline uint32_t previous_twin_draw(const PreviousTwinHistory* h, const float view_proj[16], const float camera_position[3],
                                          const float* prev_view_proj, int cut, uint32_t slot, const float model[12], float prev_mvp[16])
{
    float p[12];
    const float* pvp;
    float d[3] = {0.0f, 0.0f, 0.0f};
    int r, kept;
    if (cut || h->epoch == 0) {
        cut = 1;
        pvp = view_proj;
    } else {
        pvp = prev_view_proj ? prev_view_proj : h->view_proj;
        for (r = 0; r < 3; r++)
            d[r] = camera_position[r] - h->camera_position[r];
    }
    kept = !cut && slot < h->slots && h->rows[16 * (size_t)slot + 12] == h->epoch;
    if (kept) {
        memcpy(p, h->rows + 16 * (size_t)slot, 48);
    } else {
        memcpy(p, model, 48);
        for (r = 0; r < 3; r++)
            p[9 + r] = model[9 + r] + d[r];
    }
    instance_twin_mvp(pvp, p, prev_mvp);
    return kept ? 1u : 0u;
}

/* n records of one view; returns the kept draws */
static inline uint32_t previous_twin_many(const PreviousTwinHistory* h, const float view_proj[16], const float camera_position[3],
                                          const float* prev_view_proj, int cut, const uint32_t* slots, const float* models, uint32_t n,
                                          float* prev_mvps, uint32_t* has_history)
{
    uint32_t k, kept = 0;
    for (k = 0; k < n; k++) {
        has_history[k] = previous_twin_draw(h, view_proj, camera_position, prev_view_proj, cut, slots[k], models + 12 * (size_t)k,
                                            prev_mvps + 16 * (size_t)k);
        kept += has_history[k];
    }
    return kept;
}

#endif
