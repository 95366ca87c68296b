// Stand-alone host program around aug_records.h (no device code, no HIP runtime): builds the smallest batch of record
// kinds 3 and 4 as device_aug.build_batch_tables lays it out and runs the bounds checks over it and over broken copies.
// Meant for a host sanitizer build:  make -C hiast_amd/csrc sanitize-host
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aug_records.h"

namespace {

using namespace hiast;

int failures = 0;

void expect(int got, int want, const char* what)
{
    if (got != want) {
        std::fprintf(stderr, "FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

struct Batch {
    std::vector<int64_t> recs;
    std::vector<uint8_t> blob;       // exactly as long as its content: a read past the end is a heap overflow
};

void put_rect(Batch& b, int64_t tab, int32_t y0, int32_t y1, int32_t x0, int32_t x1)
{
    const int32_t q[4] = {y0, y1, x0, x1};
    std::memcpy(b.blob.data() + tab + 256, q, sizeof(q));
}

// sample 0: kind 3, a window of 2 x 3 in the blob (image, label, paste image, paste label, each padded to 16 bytes, then
// table + rectangle); sample 1: kind 4, the same window in a store (offsets there), table + rectangle last in the blob
Batch smallest()
{
    Batch b;
    const int ch = 2, cw = 3;
    b.recs.assign(2 * REC, -1);
    const int64_t img = 0, lbl = 32, pimg = 48, plbl = 80, tab0 = 96, tab1 = tab0 + 272;
    b.blob.assign((size_t)tab1 + HIAST_MIX_TABLE_BYTES, 1);
    int64_t* r = b.recs.data();
    r[R_KIND] = KIND_PLAN_RECT, r[R_IMG] = img, r[R_LBL] = lbl, r[R_PIMG] = pimg, r[R_PLBL] = plbl, r[R_PTAB] = tab0;
    r[R_CH] = ch, r[R_CW] = cw, r[R_FLIP] = 0;
    put_rect(b, tab0, 0, 1, 1, 3);
    r += REC;
    r[R_KIND] = KIND_STORE_RECT, r[R_IMG] = 300, r[R_LBL] = 1000, r[R_PIMG] = 2300, r[R_PLBL] = 3000, r[R_PTAB] = tab1;
    r[R_CH] = ch, r[R_CW] = cw, r[R_FLIP] = 1;
    r[R_STRIDE] = 40;
    put_rect(b, tab1, 0, 0, 0, 0);       // empty
    return b;
}

int check(const Batch& b, int max_kind)
{
    return hiast_aug_host::check_records(b.recs.data(), b.blob.data(), (int64_t)b.blob.size(), 2, max_kind);
}

}  // namespace

int main()
{
    const Batch ok = smallest();
    expect(check(ok, 4), 0, "kinds 3 and 4 through the entry that knows them");
    expect(check(ok, 2), HIAST_E_ARG, "kinds 3 and 4 through hiast_aug_geometry_store_u8");
    expect(check(ok, 1), HIAST_E_ARG, "kinds 3 and 4 through hiast_aug_geometry_u8");
    expect(check(ok, 5), HIAST_E_ARG, "a max_kind the ABI does not have");
    expect(hiast_aug_host::check_records(nullptr, ok.blob.data(), (int64_t)ok.blob.size(), 2, 4), HIAST_E_ARG, "null records");
    expect(hiast_aug_host::check_records(ok.recs.data(), nullptr, 0, 2, 4), HIAST_E_ARG, "a rectangle kind without a blob");
    const int32_t bad[][4] = {{0, 3, 0, 3}, {0, 2, 0, 4}, {-1, 2, 0, 3}, {2, 1, 0, 3}, {0, 2, 3, 2}, {0, 2, -2, 3}};
    for (const auto& q : bad)
        for (int s = 0; s < 2; ++s) {
            Batch b = smallest();
            put_rect(b, b.recs[(size_t)s * REC + R_PTAB], q[0], q[1], q[2], q[3]);
            expect(check(b, 4), HIAST_E_ARG, "a rectangle outside [0, ch] x [0, cw] or reversed");
        }
    for (size_t cut = 1; cut <= 16; cut += 3) {       // a blob too short for the last table + 16 bytes
        Batch b = smallest();
        b.blob.resize(b.blob.size() - cut);
        b.blob.shrink_to_fit();
        expect(check(b, 4), HIAST_E_ARG, "a blob that ends inside the rectangle");
    }
    {
        Batch b = smallest();
        b.blob.resize(100);                           // shorter than a table altogether
        b.blob.shrink_to_fit();
        expect(check(b, 4), HIAST_E_ARG, "a blob shorter than one table");
    }
    for (int64_t off : {(int64_t)-4, (int64_t)98, (int64_t)1 << 40, INT64_MAX - 8, INT64_MIN}) {
        Batch b = smallest();
        b.recs[R_PTAB] = off;
        expect(check(b, 4), HIAST_E_ARG, "a table offset that is negative, unaligned or far outside");
    }
    for (int w : {R_PIMG, R_PLBL, R_CH, R_CW}) {
        Batch b = smallest();
        b.recs[REC + w] = (w == R_PIMG || w == R_PLBL) ? -1 : 0;
        expect(check(b, 4), HIAST_E_ARG, "a rectangle kind without a paste source / with an empty window");
    }
    {
        Batch b = smallest();
        b.recs[R_KIND] = KIND_PLAN, b.recs[REC + R_KIND] = KIND_STORE;      // the same rows as kinds 0 and 2: nothing behind the table is read
        b.blob.resize(96 + 256);
        b.blob.shrink_to_fit();
        expect(check(b, 2), 0, "kinds 0 and 2");
        b.recs[R_KIND] = 7;
        expect(check(b, 4), HIAST_E_ARG, "an unknown kind");
        b.recs[R_KIND] = -1;
        expect(check(b, 4), HIAST_E_ARG, "a negative kind");
    }
    if (failures) return 1;
    std::puts("aug_records_check: ok");
    return 0;
}
