// Host-side checks of the K15 record tables for the mixing preprocessors (sample_aug_mix.hip): plain C++, no device code,
// so that it also compiles into a stand-alone program for a host sanitizer run (aug_mix_check_main.cpp).
// A record of kind 3 / 4 (a kind 0 / kind 2 record whose paste is confined to a rectangle) points with its paste_table
// word at 256 table bytes followed by ry0, ry1, rx0, rx1 as little-endian int32 in window coordinates.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/hiast_hip.h"

namespace hiast_mix_host {

enum { W_KIND = 0, W_PIMG = 3, W_PLBL = 4, W_PTAB = 5, W_CH = 6, W_CW = 7 };

// recs: HOST copy [B][HIAST_AUG_REC_WORDS]; blob: HOST copy of blob_bytes bytes.  0, or HIAST_E_ARG for a kind outside
// 0..max_kind, and for a record of kind 3 / 4 without a paste source, whose table + rectangle does not lie inside the blob at
// a 4-byte aligned offset, or whose rectangle leaves [0, ch] x [0, cw] or has a first edge behind its second
inline int check_records(const int64_t* recs, const uint8_t* blob, int64_t blob_bytes, int B, int max_kind)
{
    if (!recs || B <= 0 || max_kind < 0 || max_kind > HIAST_MIX_KIND_STORE_RECT) return HIAST_E_ARG;
    for (int b = 0; b < B; ++b) {
        const int64_t* r = recs + (size_t)b * HIAST_AUG_REC_WORDS;
        const int64_t kind = r[W_KIND];
        if (kind < 0 || kind > max_kind) return HIAST_E_ARG;
        if (kind != HIAST_MIX_KIND_PLAN_RECT && kind != HIAST_MIX_KIND_STORE_RECT) continue;
        const int64_t tab = r[W_PTAB], ch = r[W_CH], cw = r[W_CW];
        if (!blob || r[W_PIMG] < 0 || r[W_PLBL] < 0 || ch <= 0 || cw <= 0) return HIAST_E_ARG;
        if (tab < 0 || tab % 4 != 0 || blob_bytes < HIAST_MIX_TABLE_BYTES || tab > blob_bytes - HIAST_MIX_TABLE_BYTES)
            return HIAST_E_ARG;
        int32_t q[4];
        std::memcpy(q, blob + tab + 256, sizeof(q));
        if (q[0] < 0 || q[0] > q[1] || q[1] > ch || q[2] < 0 || q[2] > q[3] || q[3] > cw) return HIAST_E_ARG;
    }
    return 0;
}

}  // namespace hiast_mix_host
