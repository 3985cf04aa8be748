// Ordered-reduction queue of one backward: host logic only, no device code (the kernel and the producers: kernels_train.hip; a host-only program
// supplies its own red_launch_batch - tests/native/red_queue_test.cpp).  A producer writes one partial tile per split of its row range into an
// extent it takes from the queue's arena (alloc), then records a job that adds the partials into the gradient:
//   out[(i / cols) * ld_out + i % cols] += sum_{p < nparts} part[p * stride + i]     for i < split_at (columns >= cols_keep: operand padding;
//   wrap_rows: output rows beyond it continue wrap_shift columns to the right - the [Wa | Wb] blocks of a first Linear's weight gradient, produced
//   as one 256-row product);  out2[i - split_at] += ... for split_at <= i < split_at + out2_keep (the bias gradient riding behind a weight tile).
// No float atomics: gradients are bit-reproducible.  One launch runs up to RED_MAX jobs (job table by value in the kernel arguments): a kernel
// boundary costs ~4.7 us on this part and a step has ~180 of these reductions, each a few microseconds of work.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

struct RedJob {
    const float* part; float* out; float* out2; size_t stride;
    int nparts, count, cols, ld_out, split_at, cols_keep, out2_keep, wrap_rows, wrap_shift, blk0;
};
#define RED_MAX 48
struct RedBatch { RedJob j[RED_MAX]; int n; };
static_assert(sizeof(RedBatch) <= 4000, "job table travels in the kernel arguments");
// one launch of `blocks` workgroups over the jobs of b (blk0 ascending, 64 elements per workgroup): kernels_train.hip, k_reduce_batch
void red_launch_batch(const RedBatch& b, int blocks, hipStream_t s);

// rows x [p + r * ld, p + r * ld + width) floats: the partials or one output of a job
struct RedSpan { const float* p; size_t ld, rows, width; };
// never false when two spans share an element; exact when their ld is equal (different ld: true as soon as the hulls overlap)
static inline bool spans_meet(const RedSpan& a, const RedSpan& b) {
    if (!a.rows || !a.width || !b.rows || !b.width) return false;
    const long long d = ((intptr_t)b.p - (intptr_t)a.p) / (intptr_t)sizeof(float);
    const long long ha = (long long)((a.rows - 1) * a.ld + a.width), hb = (long long)((b.rows - 1) * b.ld + b.width);
    if (d >= ha || -d >= hb) return false;                 // hulls apart
    if (a.ld != b.ld) return true;
    // row i of a meets row j of b iff -b.width < d + (j - i) ld < a.width: the least m = j - i above the lower bound decides
    const long long ld = (long long)a.ld, lo = -(long long)b.width - d;
    long long m = (lo >= 0 ? lo / ld : -((-lo + ld - 1) / ld)) + 1;
    if (m < 1 - (long long)a.rows) m = 1 - (long long)a.rows;
    return m <= (long long)b.rows - 1 && d + m * ld < (long long)a.width;
}
static inline RedSpan part_span(const RedJob& J) { return RedSpan{J.part, J.stride, (size_t)J.nparts, (size_t)J.count}; }
static inline RedSpan out_span(const RedJob& J) {      // (wrap: the hull of the wrapped column blocks)
    const int rows = (J.split_at + J.cols - 1) / J.cols;
    if (!J.wrap_rows) return RedSpan{J.out, (size_t)J.ld_out, (size_t)rows, (size_t)J.cols_keep};
    return RedSpan{J.out, (size_t)J.ld_out, (size_t)std::min(rows, J.wrap_rows), (size_t)((rows - 1) / J.wrap_rows * J.wrap_shift + J.cols_keep)};
}
static inline RedSpan out2_span(const RedJob& J) {
    const size_t n = J.out2 ? (size_t)std::min(J.out2_keep, J.count - J.split_at) : 0;
    return RedSpan{J.out2, n, 1, n};
}
static inline bool outputs_meet(const RedJob& a, const RedJob& b) {
    const RedSpan sa[2] = {out_span(a), out2_span(a)}, sb[2] = {out_span(b), out2_span(b)};
    for (const RedSpan& x : sa)
        for (const RedSpan& y : sb)
            if (spans_meet(x, y)) return true;
    return false;
}

// The queue launches what it holds when the arena cannot hold the next extent, before a job whose output footprint meets a pending job's (the jobs
// of one launch add with plain +=), when the table is full, at flush (a gradient chunk becomes final) and at end; `one` launches every job on its
// own.  A request or job outside open .. end, an extent larger than the arena, a job on another stream and a job whose partials are not inside the
// extents handed out or meet a pending job's partials are refused: nothing of it is recorded and end reports false.  open starts clean: nothing a
// queue refused reaches the next backward.
struct RedQueue {
    bool active = false, one = false, bad = false;      // one: a launch per job;  bad: sticky until end reports it
    float* arena = nullptr; size_t floats = 0, used = 0;
    hipStream_t s = nullptr;
    RedBatch b{};
    int blocks = 0;

    void open(float* p, size_t n, hipStream_t stream, bool launch_per_job) {
        active = true; one = launch_per_job; bad = false;
        arena = p; floats = n; used = 0; s = stream; b.n = 0; blocks = 0;
    }
    void launch() { if (active && b.n > 0) red_launch_batch(b, blocks, s); b.n = 0; blocks = 0; }
    void flush() { launch(); used = 0; }
    bool end() {
        flush();
        const bool ok = !bad;
        active = false; bad = false;
        return ok;
    }
    float* alloc(size_t n_floats) {
        const size_t n = (n_floats + 63) & ~(size_t)63;    // (extents 256-byte aligned)
        if (!active || n > floats) { bad = true; return nullptr; }
        if (floats - used < n) flush();
        float* p = arena + used;
        used += n;
        return p;
    }
    // records the ordered reduction J (blk0 is assigned here) of a producer that launched on `stream`
    void record(RedJob J, hipStream_t stream) {
        const RedSpan ps = part_span(J);
        if (!active || stream != s || J.nparts < 1 || J.part < arena || (size_t)(J.part - arena) + ps.ld * (ps.rows - 1) + ps.width > used) {
            bad = true;
            return;
        }
        bool clash = b.n == RED_MAX;
        for (int t = 0; t < b.n; ++t) {
            if (spans_meet(part_span(b.j[t]), ps)) { bad = true; return; }
            clash = clash || outputs_meet(b.j[t], J);
        }
        if (clash) launch();                                // (not flush: this job's partials stay where they are)
        J.blk0 = blocks;
        b.j[b.n++] = J;
        blocks += (J.count + 63) / 64;
        if (one) launch();
    }
};
