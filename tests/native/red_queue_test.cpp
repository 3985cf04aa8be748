// Host-only test of the ordered-reduction queue (rna-mpnn_amd/csrc/red_queue.h): spans_meet against a brute-force element-set intersection, and what
// the queue launches, when, and what it refuses.  red_launch_batch here records the batches instead of launching a kernel; no pointer handed to the
// queue is ever dereferenced.  Built and run by tests/test_red_queue_cpu.py (address + undefined-behaviour sanitizers); exit status = failed checks.
#include "red_queue.h"
#include <cstdio>
#include <vector>

struct Launch { RedBatch b; int blocks; hipStream_t s; };
static std::vector<Launch> g_launches;
void red_launch_batch(const RedBatch& b, int blocks, hipStream_t s) { g_launches.push_back(Launch{b, blocks, s}); }

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { if (++g_failed <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static float g_arena[1 << 16], g_grad[1 << 16];       // addresses only
static hipStream_t const STREAM = (hipStream_t)(g_grad + 1), OTHER = (hipStream_t)(g_grad + 2);

// a one-row job: `count` elements of `nparts` partials at `part` (stride = count) added into out[0 .. count)
static RedJob job(const float* part, int nparts, int count, float* out) {
    return RedJob{part, out, nullptr, (size_t)count, nparts, count, count, count, count, count, count, 0, 0, 0};
}
static RedQueue fresh(size_t floats = sizeof(g_arena) / sizeof(float), bool one = false) {
    g_launches.clear();
    RedQueue q;
    q.open(g_arena, floats, STREAM, one);
    return q;
}

static void test_spans_meet() {
    static float buf[256];
    float* const base = buf + 128;
    long long pairs = 0;
    for (int ar = 0; ar <= 4; ++ar) for (int aw = 0; aw <= 5; ++aw) for (int ald = aw; ald <= 8; ++ald)
    for (int br = 0; br <= 4; ++br) for (int bw = 0; bw <= 5; ++bw) for (int bld = bw; bld <= 8; ++bld)
    for (int d = -24; d <= 24; ++d) {
        bool in_a[128] = {};
        for (int r = 0; r < ar; ++r) for (int c = 0; c < aw; ++c) in_a[32 + r * ald + c] = true;
        bool hit = false;
        for (int r = 0; r < br; ++r) for (int c = 0; c < bw; ++c) hit = hit || in_a[32 + d + r * bld + c];
        const RedSpan a{base, (size_t)ald, (size_t)ar, (size_t)aw}, b{base + d, (size_t)bld, (size_t)br, (size_t)bw};
        const bool meet = spans_meet(a, b);
        const bool empty = !ar || !aw || !br || !bw;
        const long long ha = (ar - 1) * ald + aw, hb = (br - 1) * bld + bw;
        const bool hulls = !empty && d < ha && -d < hb;
        if (hit) CHECK(meet);                            // never "apart" when elements intersect
        if (ald == bld || empty) CHECK(meet == hit);     // exact with equal ld (and for empty spans)
        if (meet) CHECK(hulls);                          // the conservative answer needs overlapping hulls
        CHECK(spans_meet(b, a) == meet);                 // the answer does not depend on the order
        ++pairs;
    }
    std::printf("spans_meet: %lld pairs\n", pairs);
}

static void test_batching() {
    RedQueue q = fresh();
    const float* parts[RED_MAX + 1];
    int counts[RED_MAX + 1];
    for (int i = 0; i <= RED_MAX; ++i) {
        counts[i] = 1 + (37 * i) % 200;                  // 1 .. 200 elements: one to four workgroups
        float* p = q.alloc(2 * (size_t)counts[i]);
        parts[i] = p;
        CHECK(p != nullptr);
        if (i == RED_MAX) CHECK(g_launches.empty());     // RED_MAX disjoint jobs: one batch, still pending
        q.record(job(p, 2, counts[i], g_grad + 256 * i), STREAM);
    }
    CHECK(g_launches.size() == 1);                       // the RED_MAX + 1-th job pushed the first RED_MAX out
    if (g_launches.size() == 1) {
        const Launch& L = g_launches[0];
        CHECK(L.b.n == RED_MAX && L.s == STREAM);
        int blocks = 0;
        for (int t = 0; t < L.b.n && t < RED_MAX; ++t) {
            CHECK(L.b.j[t].part == parts[t] && L.b.j[t].count == counts[t]);      // recording order
            CHECK(L.b.j[t].blk0 == blocks);                                       // ascending, dense
            blocks += (counts[t] + 63) / 64;
        }
        CHECK(L.blocks == blocks);
    }
    CHECK(q.b.n == 1 && q.b.j[0].part == parts[RED_MAX] && q.b.j[0].blk0 == 0);
    CHECK(q.end());
    CHECK(g_launches.size() == 2 && g_launches[1].b.n == 1 && g_launches[1].blocks == (counts[RED_MAX] + 63) / 64);
}

// `pending` is recorded first; `next` must (or must not) force its launch before being recorded itself
static void expect_clash(const char* what, RedJob pending, RedJob next, bool clash) {
    const int failed = g_failed;
    RedQueue q = fresh();
    float* p0 = q.alloc(4096);
    float* p1 = q.alloc(4096);
    pending.part = p0; next.part = p1;
    q.record(pending, STREAM);
    const size_t used = q.used;
    q.record(next, STREAM);
    if (clash) {
        CHECK(g_launches.size() == 1 && g_launches[0].b.n == 1 && g_launches[0].b.j[0].part == p0);
        CHECK(q.b.n == 1 && q.b.j[0].part == p1 && q.b.j[0].blk0 == 0);
    } else {
        CHECK(g_launches.empty() && q.b.n == 2);
    }
    CHECK(q.used == used && used == 8192);               // launched, not flushed: the new job's partials stay valid
    CHECK(q.end());
    if (g_failed > failed) std::printf("  (case: %s)\n", what);
}
static void test_overlapping_outputs() {
    float* W = g_grad;
    expect_clash("same out", job(nullptr, 2, 128, W), job(nullptr, 2, 128, W), true);
    expect_clash("out tail", job(nullptr, 2, 128, W), job(nullptr, 2, 64, W + 127), true);
    expect_clash("adjacent out", job(nullptr, 2, 128, W), job(nullptr, 2, 64, W + 128), false);
    // 4 x 16 tile into rows of 64: columns 16 .. 63 of each row are free for another job
    RedJob tile = job(nullptr, 2, 64, W);
    tile.cols = 16; tile.cols_keep = 16; tile.ld_out = 64;
    RedJob gap = job(nullptr, 2, 48, W + 16);            // (same row stride: with another one the answer is the hulls')
    gap.ld_out = 64;
    expect_clash("between the rows of a strided tile", tile, gap, false);
    gap.out = W + 32;                                    // 32 .. 79: into row 1 (64 .. 79)
    expect_clash("into a row of a strided tile", tile, gap, true);
    // out2 (a bias gradient behind the weight tile): elements split_at .. count go to out2
    RedJob bias = job(nullptr, 2, 128 + 16, W + 1024);
    bias.split_at = 128; bias.cols = 128; bias.cols_keep = 128; bias.ld_out = 128; bias.out2 = W + 64; bias.out2_keep = 16;
    expect_clash("out2 meets a pending out", job(nullptr, 2, 128, W), bias, true);
    expect_clash("out meets a pending out2", bias, job(nullptr, 2, 8, W + 72), true);
    bias.out2 = W + 128;
    expect_clash("out2 beside a pending out", job(nullptr, 2, 128, W), bias, false);
    // wrap: 4 rows x 8 columns, rows 2 .. 3 continue 8 columns to the right of rows 0 .. 1 (ld_out 32): footprint = rows 0 .. 1 x columns 0 .. 15
    RedJob wrap = job(nullptr, 2, 32, W);
    wrap.cols = 8; wrap.cols_keep = 8; wrap.ld_out = 32; wrap.wrap_rows = 2; wrap.wrap_shift = 8;
    RedJob blk = job(nullptr, 2, 8, W + 8);              // columns 8 .. 15 of row 0: only the wrapped rows 2 .. 3 land there
    blk.ld_out = 32;
    expect_clash("wrapped block meets a pending out", blk, wrap, true);
    expect_clash("pending wrapped block", wrap, job(nullptr, 2, 8, W + 32 + 8), true);
    expect_clash("rows the wrap folded away", job(nullptr, 2, 8, W + 64), wrap, false);
}

static void test_arena() {
    RedQueue q = fresh(1024);
    float* a = q.alloc(100);
    CHECK(a == g_arena && q.used == 128);                // extents rounded to 64 floats
    CHECK(q.alloc(1) == g_arena + 128 && q.used == 192);
    q.record(job(a, 4, 25, g_grad), STREAM);
    CHECK(g_launches.empty());
    CHECK(q.alloc(833) == g_arena && q.used == 896);     // 896 > 832 left: what is pending runs, the arena restarts at 0
    CHECK(g_launches.size() == 1 && g_launches[0].b.n == 1 && q.b.n == 0);
    CHECK(q.alloc(128) == g_arena + 896 && q.used == 1024 && g_launches.size() == 1);      // an exact fit does not flush
    CHECK(q.alloc(1024) == g_arena && q.used == 1024);   // the whole arena is a valid extent
    CHECK(q.end());
}

static void test_refusals() {
    {   // larger than the arena
        RedQueue q = fresh(1024);
        CHECK(q.alloc(1025) == nullptr && q.used == 0);
        CHECK(!q.end() && g_launches.empty());
        q.open(g_arena, 1024, STREAM, false);
        CHECK(q.end());
    }
    {   // another stream
        RedQueue q = fresh();
        float* p = q.alloc(128);
        q.record(job(p, 2, 64, g_grad), OTHER);
        CHECK(q.b.n == 0);
        CHECK(!q.end() && g_launches.empty());
    }
    {   // partials outside the extents handed out: past the end, before the arena, no partials at all
        for (int v = 0; v < 3; ++v) {
            g_launches.clear();
            RedQueue q;
            q.open(g_arena + 1024, 4096, STREAM, false);
            float* p = q.alloc(128);
            q.record(v == 0 ? job(p, 2, 65, g_grad) : v == 1 ? job(g_arena + 960, 2, 64, g_grad) : job(p, 0, 64, g_grad), STREAM);
            CHECK(q.b.n == 0);
            CHECK(!q.end() && g_launches.empty());
        }
    }
    {   // partials that meet a pending job's partials: the pending job still runs, the refused one does not
        RedQueue q = fresh();
        float* p = q.alloc(128);
        q.record(job(p, 1, 64, g_grad), STREAM);
        q.record(job(p + 32, 1, 64, g_grad + 4096), STREAM);
        CHECK(q.b.n == 1);
        CHECK(!q.end());
        CHECK(g_launches.size() == 1 && g_launches[0].b.n == 1 && g_launches[0].b.j[0].part == p);
    }
    {   // outside open .. end
        g_launches.clear();
        RedQueue q;
        CHECK(q.alloc(64) == nullptr);
        q.record(job(g_arena, 1, 64, g_grad), STREAM);
        CHECK(q.b.n == 0 && !q.end() && g_launches.empty());
        CHECK(q.end());                                  // end reported it: clean again
    }
    {   // a call that returned between open and end after a refusal: the next open starts clean
        RedQueue q = fresh(1024);
        CHECK(q.alloc(4096) == nullptr && q.bad);
        q.open(g_arena, 1024, STREAM, false);
        float* p = q.alloc(64);
        q.record(job(p, 1, 64, g_grad), STREAM);
        CHECK(q.end() && g_launches.size() == 1);
    }
}

static void test_launch_per_job() {
    RedQueue q = fresh(sizeof(g_arena) / sizeof(float), true);
    for (int i = 0; i < 5; ++i) {
        float* p = q.alloc(256);
        q.record(job(p, 2, 100, g_grad + 128 * i), STREAM);
        CHECK((int)g_launches.size() == i + 1 && q.b.n == 0);
        if ((int)g_launches.size() == i + 1) CHECK(g_launches[i].b.n == 1 && g_launches[i].b.j[0].part == p && g_launches[i].b.j[0].blk0 == 0 && g_launches[i].blocks == 2);
    }
    CHECK(q.end() && g_launches.size() == 5);
}

int main() {
    test_spans_meet();
    test_batching();
    test_overlapping_outputs();
    test_arena();
    test_refusals();
    test_launch_per_job();
    std::printf(g_failed ? "red_queue_test: %d checks FAILED\n" : "red_queue_test: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
