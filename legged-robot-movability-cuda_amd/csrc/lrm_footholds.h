// lrm_footholds.h -- the foothold choice of lrm_footholds_dev / lrm_footholds_cpu, shared by the kernel and the host loop
// so that both order candidates by the same bits.  Compiled with -ffp-contract=off: d2 is three separate f32 products
// and two separate f32 adds, in this order, on both sides.
#pragma once
#include <stdint.h>
#include "lrm_point.h" // LrmVec3

// The caller's nominal foot offsets (host nlegs x 3, NULL = zero), passed to the kernel by value.
struct LrmFootNominal {
    float v[LRM_MAX_LEGS][3];
};

// d2 of target t from the nominal point c = body + nominal (one f32 add per component)
LRM_HD float lrm_foothold_d2(LrmVec3 t, LrmVec3 body, const float nominal[3]) {
    const float cx = body.x + nominal[0], cy = body.y + nominal[1], cz = body.z + nominal[2];
    const float dx = t.x - cx, dy = t.y - cy, dz = t.z - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Candidate key: d2 >= 0, so its bits order like its value; ties go to the smaller index.  No candidate = ~0.
LRM_HD uint64_t lrm_foothold_key(float d2, uint32_t index) {
    union {
        float f;
        uint32_t u;
    } bits;
    bits.f = d2;
    return ((uint64_t)bits.u << 32) | index;
}
constexpr uint64_t kLrmFootholdNone = ~(uint64_t)0;
// What a key holds: the candidate's index and d2, or -1 and +inf when there is none (have false: the key is not read).
struct LrmFootholdChoice {
    int32_t index;
    float d2;
};
LRM_HD LrmFootholdChoice lrm_foothold_key_decode(uint64_t key, bool have) {
    union {
        uint32_t u;
        float f;
    } bits;
    bits.u = (uint32_t)(key >> 32);
    return LrmFootholdChoice{have ? (int32_t)(uint32_t)key : -1, have ? bits.f : __builtin_inff()};
}
