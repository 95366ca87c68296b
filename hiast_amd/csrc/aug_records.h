// The K15 sample record (one int64 row per sample, include/hiast_hip.h) as every C source reads it: the word indices and the
// kinds, defined once, and the host-side check of a batch of records.  Plain C++, no device code, so that it also compiles
// into a stand-alone program for a host sanitizer run (aug_records_check_main.cpp).
// A record of kind 3 / 4 (a kind 0 / kind 2 record whose paste is confined to a rectangle) points with its paste_table
// word at 256 table bytes followed by ry0, ry1, rx0, rx1 as little-endian int32 in window coordinates.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/hiast_hip.h"

namespace hiast {

enum { R_KIND, R_IMG, R_LBL, R_PIMG, R_PLBL, R_PTAB, R_CH, R_CW, R_FLIP, R_HLO, R_HN, R_HK, R_HT, R_VLO, R_VN, R_VK, R_VT,
       R_NX, R_NY, R_STRIDE };
enum { KIND_PLAN = 0, KIND_FINISHED = 1, KIND_STORE = HIAST_STORE_KIND, KIND_PLAN_RECT = HIAST_MIX_KIND_PLAN_RECT,
       KIND_STORE_RECT = HIAST_MIX_KIND_STORE_RECT };
static_assert(R_STRIDE == HIAST_STORE_REC_STRIDE && R_STRIDE < HIAST_AUG_REC_WORDS, "the stride is the record's spare word");
constexpr int REC = HIAST_AUG_REC_WORDS;

}  // namespace hiast

namespace hiast_aug_host {

// recs: HOST copy [B][HIAST_AUG_REC_WORDS]; blob: HOST copy of blob_bytes bytes.  0, or HIAST_E_ARG for a kind outside
// 0..max_kind, and for a record of kind 3 / 4 without a paste source, whose table + rectangle does not lie inside the blob at
// a 4-byte aligned offset, or whose rectangle leaves [0, ch] x [0, cw] or has a first edge behind its second
inline int check_records(const int64_t* recs, const uint8_t* blob, int64_t blob_bytes, int B, int max_kind)
{
    using namespace hiast;
    if (!recs || B <= 0 || max_kind < 0 || max_kind > KIND_STORE_RECT) return HIAST_E_ARG;
    for (int b = 0; b < B; ++b) {
        const int64_t* r = recs + (size_t)b * REC;
        const int64_t kind = r[R_KIND];
        if (kind < 0 || kind > max_kind) return HIAST_E_ARG;
        if (kind != KIND_PLAN_RECT && kind != KIND_STORE_RECT) continue;
        const int64_t tab = r[R_PTAB], ch = r[R_CH], cw = r[R_CW];
        if (!blob || r[R_PIMG] < 0 || r[R_PLBL] < 0 || ch <= 0 || cw <= 0) return HIAST_E_ARG;
        if (tab < 0 || tab % 4 != 0 || blob_bytes < HIAST_MIX_TABLE_BYTES || tab > blob_bytes - HIAST_MIX_TABLE_BYTES)
            return HIAST_E_ARG;
        int32_t q[4];
        std::memcpy(q, blob + tab + 256, sizeof(q));
        if (q[0] < 0 || q[0] > q[1] || q[1] > ch || q[2] < 0 || q[2] > q[3] || q[3] > cw) return HIAST_E_ARG;
    }
    return 0;
}

}  // namespace hiast_aug_host
