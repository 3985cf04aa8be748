// rnampnn_design_dfa_profile: INFERENCE next to the draws of rnampnn_design_dfa, as design_profile.hip stands next to rnampnn_design_count
// and rnampnn_design_avoid.  In one launch and in fp64 it returns the exact distribution that entry samples from - per-position marginals
// P(x_t = c), log_z = l_0(0), the free log partition sum and the entropy - together with the draw entry's own `infeasible` and `dfa_miss`,
// on automata of up to 256 states and with the backward table l_t(a) in the caller's WORKSPACE in global memory, [b][t][live column], so
// LDS grows with T alone.  The contract is the one include/rnampnn_hip.h documents and tests/_design_dfa_profile_ref.py restates.
// One 256-thread workgroup per RNA, thread = state.  (A) the fp64 rows, the masks and the free sum; the automaton (dfa_chain_dev.h).
// (B) k_design_dfa's backward pass (dfa_rows_init, dfa_backward): l_{t+1} and l_t in two LDS rows, every live l_t(a) to the workspace.
// (C) the forward walk in the POSTERIOR domain.  With q_t(a) = exp(alpha_t(a) + l_t(a) - log_z), the probability that the draw is in
// state a before position t, the cell (a, c) carries w = q_t(a) exp(z_t(c) + l_{t+1}(delta(a,c)) - l_t(a)) - q times the very
// conditional the draw entry selects with - and P_t(c) = the sum of w over a, q_{t+1}(a') = the sum of w over the cells that lead to a'.
// That is the header's alpha recursion multiplied through by exp(l - log_z); every number lies in [0, 1], so the walk needs no maxima and
// no logarithm: four exps per thread and step.  What underflows is a state whose posterior is below 1e-308.  q_t(a) lives in the
// register of thread a; l_t(a) and the four l_{t+1}(delta(a, c)) come from the workspace (written by this workgroup: a barrier orders
// them; they do not depend on q, so they are loaded at the top of the step before).
//   The marginals of a step.  The 1,024 cells are parked in LDS class-major (cell = 256 c + a: a wave writes and reads consecutive
//   doubles); wave c adds column c, four doubles per lane and a butterfly, and its lane 0 writes P_t(c) and keeps the sum of P z.
//   The scatter along delta is a SEGMENTED SUM over the cells sorted by target.  Once per RNA a counting sort (thread = target over the
//   sources in state order, a workgroup scan of the counts) lists the live cells by (target, source, class); thread j owns the sorted
//   positions 4 j .. 4 j + 3.  Where a segment starts and ends is the automaton's, so every branch of the scan is a bit of one register:
//   the thread adds its four cells with restarts at the heads, the wave scans the threads' open ends in six shuffles whose "add" bits
//   were found once, the four wave totals cross in LDS, and the thread that owns the last cell of a segment writes q_{t+1}(target).
//   Three barriers, six double shuffles and at most seven additions per thread and step WHATEVER the in-degree of a state - the root
//   of an Aho-Corasick automaton collects several hundred of the cells - and one fixed order of addition, so two calls give the same bytes.
// With dfa_miss = 1 there is no chain: all threads write the per-position softmax over the admitted classes (pf_softmax_rows).
//   LDS bytes(T) = 32 T + 16 ceil(T / 16) + 15,392: the fp64 rows and the masks; 8,208 for the cells (the two rows of l lie over them
//   during (B)), 2,048 for q_{t+1}, 3,088 for the sorted cells and their targets, 1,792 for the automaton, 256 for the sums, the scans
//   and the reduction's scratch.  160 KiB holds T <= 4,498 at every automaton.
// Non-finite rows can make the outputs of THAT RNA NaN; no index depends on a value, so nothing faults and no other RNA changes.
#include "dfa_chain_dev.h"
#include "profile_dev.h"

namespace {
using DfaPfArgs = DfaChainArgs<DesignArgs, PfOut>;      // tab: (B,T,live); more: the profile's outputs

constexpr int DP_CELLS = 4 * DFA_MAX_STATES;                       // 1,024 cells (a, c), cell = 256 c + a; cell 1,024 holds 0 for the padding
constexpr size_t DP_FIXED = 8 * (DP_CELLS + 2) + 8 * DFA_MAX_STATES + 8 * SC_WAVES + 8 * 3 * SC_WAVES + 4 * DFA_MAX_STATES + 2 * DP_CELLS +
                            (DP_CELLS + 16) + 2 * DFA_MAX_STATES + DFA_MAX_STATES + 2 * 4 * SC_WAVES + DFA_LDS_SCRATCH;
static_assert(DP_FIXED == 15392, "the bytes include/rnampnn_hip.h gives");

// bits of a thread's scan register: 0..3 a head at its cell e, 4..7 a tail, 8..11 the carry reaches cell e, 12..17 the wave scan adds at
// step k, 18 a head in an earlier thread of the wave, 19..20 the earlier waves whose totals reach this one
constexpr int DP_HEAD = 0, DP_TAIL = 4, DP_CARRY = 8, DP_ADD = 12, DP_EXCL = 18, DP_PREV = 19;

__global__ void __launch_bounds__(SC_THREADS) k_design_dfa_profile(DfaPfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dpf_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live, lane = tid & 63, wave = tid >> 6;
    double* zs = reinterpret_cast<double*>(dpf_lds);                               // [T][4]      z of a position
    double* cand = zs + 4 * (size_t)T;                                             // [1026]      w of a cell, class-major; [1024] = 0
    double* row = cand;                                                            // [2][256]    l_{t+1} and l_t by state, during (B) only
    double* qn = cand + DP_CELLS + 2;                                              // [256]       q_{t+1} by state
    double* wtot = qn + DFA_MAX_STATES;                                            // [4]         the open end of a wave's scan
    double (*s_d)[SC_WAVES] = reinterpret_cast<double (*)[SC_WAVES]>(wtot + SC_WAVES);
    unsigned* nx = reinterpret_cast<unsigned*>(s_d + 3);                           // [256]       delta(a, .), a byte per class
    unsigned short* perm = reinterpret_cast<unsigned short*>(nx + DFA_MAX_STATES); // [1024]      the cell at a sorted position
    unsigned char* stg = reinterpret_cast<unsigned char*>(perm + DP_CELLS);        // [1040]      its target
    unsigned short* own = reinterpret_cast<unsigned short*>(stg + DP_CELLS + 16);  // [256]       the column of state a, or DFA_DEAD
    unsigned char* kd = reinterpret_cast<unsigned char*>(own + DFA_MAX_STATES);    // [256]       bit 0 dead, bit 1 accepting
    int* s_cnt = reinterpret_cast<int*>(kd + DFA_MAX_STATES);                      // [4]         the cells of a wave's targets
    int* s_head = s_cnt + SC_WAVES;                                                // [4]         a segment starts in the wave
    unsigned char* red = reinterpret_cast<unsigned char*>(s_head + SC_WAVES);      // the reduction's scratch
    const DsScratch sc = ds_scratch(red);
    unsigned char* ms = red + DFA_LDS_SCRATCH;                                     // [T]         the mask of a position
    double* tab = a.tab + (size_t)b * T * AL;                                      // [T][AL]     l_t of a live state
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    // ---- A: the automaton (first: its 512 bits of launch arguments are not held across the row loop); rows, masks and the free sum
    const DfaState me = dfa_load_state(a, A, tid, DFA_DEAD, own, kd);
    const bool live = me.live, accepts = me.accepts;
    int bad = 0;
    double free_sum = 0.0;
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad);
    for (int t = tid; t < n; t += SC_THREADS) {                                    // (a loop of its own: the scalar registers of the two do not add up)
        const double z[4] = {zs[4 * t], zs[4 * t + 1], zs[4 * t + 2], zs[4 * t + 3]};
        free_sum += ds_lse<4>(z, 15);
    }
    dfa_rows_init(row, n, tid, accepts);
    __syncthreads();
    int cc[4], ck[4], ok = 0;
    dfa_load_delta(a, tid, DFA_DEAD, own, nx, [&](int c, unsigned nxt, unsigned k) {
        ok |= (k != DFA_DEAD ? 1 : 0) << c;
        cc[c] = k != DFA_DEAD ? (int)nxt : 0;                                      // (the LDS rows are indexed by state,
        ck[c] = k != DFA_DEAD ? (int)k : 0;                                        //  the workspace by live column)
    });
    __syncthreads();
    int accm = 0;                                                                  // the classes that lead into a live accepting state
#pragma unroll
    for (int c = 0; c < 4; ++c) accm |= (((ok >> c) & 1) && (kd[cc[c]] & 2) ? 1 : 0) << c;
    // ---- B: l_t(a), t = n-1 .. 0: k_design_dfa's backward pass (dfa_chain_dev.h)
    const int mine = own[tid];
    const bool miss = dfa_backward(zs, ms, row, tab, own, n, AL, tid, live, cc, ok);
    const double log_z = n > 0 && !miss ? row[0] : 0.0;
    __syncthreads();                                                // the rows of l make way for the cells
    double pz_sum = 0.0, lz_sum = 0.0;
    if (miss) {
        // ---- C': no admitted sequence is accepted: the per-position softmax over the admitted classes, as the draw falls back to
        pf_softmax_rows(a.more.marg, zs, ms, pad0, n, tid, pz_sum, lz_sum);
    } else if (n > 0) {
        // ---- C, once: the live cells sorted by (target, source, class).  Thread = target counts its cells, a workgroup scan of the counts
        // gives its first position, a second pass lists them.
        auto over_sources = [&](auto visit) {
            if (!live) return;
            for (int s = 0; s < A; ++s) {
                const unsigned w = nx[s];
                if (kd[s] & 1) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (((w >> (8 * c)) & 255u) == (unsigned)tid) visit(DFA_MAX_STATES * c + s);
            }
        };
        int cnt = 0;
        over_sources([&](int) { ++cnt; });
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_cnt[wave] = incl;
        qn[tid] = 0.0;                                              // a state no live cell leads to keeps q = 0
        if (tid == 0) cand[DP_CELLS] = 0.0;
        __syncthreads();
        int at = incl - cnt, N = 0;
#pragma unroll
        for (int w = 0; w < SC_WAVES; ++w) {
            at += w < wave ? s_cnt[w] : 0;
            N += s_cnt[w];
        }
        over_sources([&](int cell) { perm[at] = (unsigned short)cell; stg[at] = (unsigned char)tid; ++at; });
        for (int p = N + tid; p < DP_CELLS; p += SC_THREADS) { perm[p] = (unsigned short)DP_CELLS; stg[p] = 0; }
        __syncthreads();
        // thread j owns the sorted positions 4 j .. 4 j + 3; a position past N is a segment of its own that holds 0 and ends nowhere
        unsigned pm[4], tg[4], bits = 0;
        {
            bool headed = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 4 * tid + e;
                pm[e] = perm[p];
                tg[e] = stg[p];
                const bool real = p < N;
                const bool head = !real || p == 0 || stg[p > 0 ? p - 1 : 0] != tg[e];
                const bool tail = real && (p == N - 1 || stg[p + 1] != tg[e]);
                headed = headed || head;
                bits |= (head ? 1u : 0u) << (DP_HEAD + e) | (tail ? 1u : 0u) << (DP_TAIL + e) | (headed ? 0u : 1u) << (DP_CARRY + e);
            }
            int f = headed ? 1 : 0;
            const unsigned long long heads = __ballot(headed);
            if (lane == 0) s_head[wave] = heads != 0ull ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int pf = __shfl_up(f, 1 << k, 64);
                if (lane >= (1 << k)) {
                    bits |= (f ? 0u : 1u) << (DP_ADD + k);
                    f |= pf;
                }
            }
            const int before = __shfl_up(f, 1, 64);
            bits |= (lane > 0 && before ? 1u : 0u) << DP_EXCL;
            __syncthreads();
            unsigned prev = 0;                                      // the waves before this one up to and with the last that holds a head
            for (int w = wave - 1; w >= 0; --w) {
                ++prev;
                if (s_head[w]) break;
            }
            bits |= prev << DP_PREV;
        }
        // ---- C: the forward walk
        double q = tid == 0 ? 1.0 : 0.0;
        double L[4], lo;
        auto load = [&](int t, double (&Lt)[4], double& lt) {
            const double* cur = tab + (size_t)t * AL;
            lt = live ? cur[mine] : -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; ++c) Lt[c] = t + 1 < n ? cur[AL + ck[c]] : ((accm >> c) & 1) ? 0.0 : -INFINITY;
        };
        load(0, L, lo);
        for (int t = 0; t < n; ++t) {
            double Ln[4] = {0.0, 0.0, 0.0, 0.0}, ln = 0.0;
            if (t + 1 < n) load(t + 1, Ln, ln);
            const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
            const double z[4] = {z01.x, z01.y, z23.x, z23.y};
            const int m = (int)ms[t] & ok;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = ((m >> c) & 1) && L[c] > -INFINITY && q > 0.0;
                cand[DFA_MAX_STATES * c + tid] = in ? q * exp(z[c] + L[c] - lo) : 0.0;
            }
            __syncthreads();
            {
                const double* colm = cand + DFA_MAX_STATES * wave;  // wave c adds the cells of class c
                const double p = sc_wave_sum(((colm[lane] + colm[64 + lane]) + colm[128 + lane]) + colm[192 + lane]);
                if (lane == 0) {
                    if (a.more.marg) a.more.marg[4 * (pad0 + t) + wave] = p;
                    pz_sum += pf_pz(p, zs[4 * t + wave]);
                }
            }
            if (t + 1 == n) break;
            double part[4], run = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double v = cand[pm[e]];
                run = ((bits >> (DP_HEAD + e)) & 1u) ? v : run + v;
                part[e] = run;
            }
            double open = run;                                      // the thread's open end; then the wave's inclusive segmented scan
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double pv = __shfl_up(open, 1 << k, 64);
                if ((bits >> (DP_ADD + k)) & 1u) open += pv;
            }
            if (lane == 63) wtot[wave] = open;
            double carry = __shfl_up(open, 1, 64);
            if (lane == 0) carry = 0.0;
            __syncthreads();
            if (!((bits >> DP_EXCL) & 1u)) {
                const int prev = (int)((bits >> DP_PREV) & 3u);
                for (int j = 1; j <= prev; ++j) carry += wtot[wave - j];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((bits >> (DP_TAIL + e)) & 1u) qn[tg[e]] = ((bits >> (DP_CARRY + e)) & 1u) ? part[e] + carry : part[e];
            __syncthreads();
            q = qn[tid];
            lo = ln;
#pragma unroll
            for (int c = 0; c < 4; ++c) L[c] = Ln[c];
        }
    }
    pf_finish(a.more, a, a.dfa_miss, miss ? 1 : 0, b, n, tid, bad, free_sum, pz_sum, lz_sum, miss, log_z, sc, s_d);
}

// the bytes of dynamic LDS, from T alone: the formula include/rnampnn_hip.h gives
size_t dpf_lds_bytes(long long T) {
    const size_t t = (size_t)T;
    return 32 * t + 16 * ((t + 15) / 16) + DP_FIXED;
}
}  // namespace

extern "C" size_t rnampnn_design_dfa_profile_workspace_bytes(int32_t B, int32_t T, int32_t n_live) {
    if (B <= 0 || T <= 0 || n_live <= 0) return 0;
    return (size_t)8 * (size_t)B * (size_t)T * (size_t)n_live;
}

extern "C" int rnampnn_design_dfa_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                          float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                          int32_t bias_per_position, const uint8_t* delta, const uint8_t* kind, int32_t n_states,
                                          void* workspace, size_t workspace_bytes, double* marginals, double* log_z, double* log_z_free,
                                          double* entropy, int32_t* infeasible, int32_t* dfa_miss, void* stream) {
    const char* name = "rnampnn_design_dfa_profile";
    const PfAsked asked{name, marginals, log_z, log_z_free, entropy, infeasible, dfa_miss};
    DfaPfArgs a{};
    const int rc = dfa_prepare(name, logits, n_rows, mask, cu_seqlens, B, T, temperature, 1, 0, nullptr, allowed, partner, wobble, bias,
                               bias_per_position, nullptr, nullptr, infeasible, delta, kind, n_states, workspace, workspace_bytes, nullptr, nullptr,
                               dfa_miss, true, a, [&] { return asked.aligned(); }, [&](int live, char* what, size_t len) {
        std::snprintf(what, len, "the table of partition sums at (B = %d, T = %d, %d live states) needs", (int)B, (int)T, live);
        return rnampnn_design_dfa_profile_workspace_bytes(B, T, live);
    });
    if (rc != RNAMPNN_OK) return rc;
    if (asked.nothing()) return RNAMPNN_OK;
    const size_t lds = dpf_lds_bytes(T);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d needs %zu bytes of LDS for the rows and the cells of a step, the limit is %zu "
                    "(T <= %lld; the table of partition sums is in the workspace and does not count)", name, (int)T, lds, DS_LDS_MAX,
                    ds_max_T([](long long t) { return dpf_lds_bytes(t); }));
    a.more = asked.out();
    return ds_launch<k_design_dfa_profile>(dim3(B), lds, stream, a);
}
