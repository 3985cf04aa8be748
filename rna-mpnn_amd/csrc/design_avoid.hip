// rnampnn_design_avoid: constrained design conditioned EXACTLY on the sequence containing none of a set of forbidden substrings, in one
// launch.  The motifs come as an Aho-Corasick DFA with the failure links compiled out (rnampnn/utils/motifs.py): `delta` (A,4) the next
// state per class, `terminal` the states in which a motif has just ended.  The model's distribution is a product over positions, so the
// conditional on "the automaton never enters a terminal state" is a chain over (position x automaton state): a backward pass of log
// partition sums l_t(a), then one forward walk per sample that draws class c in state a with weight exp(z_t(c) + l_{t+1}(delta(a,c))).
// Base pairs couple distant positions and are refused by the entry (an exact chain would carry the class of every open pair in its state).
// The contract is the one include/rnampnn_hip.h documents and tests/_design_avoid_ref.py restates; all of the draw is fp64.
// One 256-thread workgroup per RNA.  (A) every thread: the fp64 rows and the masks of the RNA into LDS; the threads below A: the
// automaton's rows, as raw next states and as the table columns of the live ones.  (B) one wave, lane = state: l_t for t = n-1 .. 0 into
// the LDS table [t][live state]; the recursion is sequential in t, so a step is four table reads issued together, one logsumexp and one
// write, with the lane's row of delta in registers and a wave-level fence between steps (no workgroup barrier).  (C) 64 samples at a
// time, one lane per sample: the forward walk, 2 bits per position into LDS words the lane owns (one write per 16 positions), then per
// sample the rows, the NLL and the counts as k_design writes and reduces them (ds_write_rows).  64 and not 256 samples at a time: the
// draws of a chunk cost 16 bytes of LDS per position, which the table needs more.  No workspace, no atomics, no host synchronisation.
// The automaton's constants and arguments, the entry's checks and the bytes of the rows are avoid_chain_dev.h's, shared with the profile.
#include "avoid_chain_dev.h"

namespace {
constexpr int AV_CHUNK = 64;                   // samples that walk together: one wave
constexpr size_t AV_LDS_SCRATCH = 96;          // the reduction's DS_SCRATCH bytes, padded
static_assert(DS_SCRATCH <= AV_LDS_SCRATCH, "the reduction's scratch");

struct AvArgs : AvChainArgs {
    int S, words;                // samples, 32-bit words of one sample's draws
    int32_t* hits;               // (S,B) or null
    int32_t* miss;               // (B) or null
};

// the words of one sample's draws: 2 bits per position, an odd count (lanes a word stride apart fall into different banks)
__host__ __device__ inline int av_words(int T) { return ((T + 15) / 16) | 1; }

__global__ void __launch_bounds__(SC_THREADS) k_design_avoid(AvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char av_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live, W = a.words;
    double* zs = reinterpret_cast<double*>(av_lds);                                // [T][4]      z of a position
    double* tab = zs + 4 * (size_t)T;                                              // [T][AL]     l_t of a live state
    unsigned* draws = reinterpret_cast<unsigned*>(tab + (size_t)AL * T);           // [64][W]     a chunk's draws
    unsigned* nx = draws + AV_CHUNK * W;                                           // [64]        delta(a, .), a byte per class
    unsigned* col = nx + AV_MAX_STATES;                                            // [64]        the table column of delta(a, .), or AV_DEAD
    int* hitc = reinterpret_cast<int*>(col + AV_MAX_STATES);                       // [64]        a chunk's hits
    unsigned char* red = reinterpret_cast<unsigned char*>(hitc + AV_CHUNK);        // the reduction's scratch
    const DsScratch sc = ds_scratch(red);
    unsigned char* ms = red + AV_LDS_SCRATCH;                                      // [T]         the mask of a position
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const unsigned long long term = a.terminal;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    // ---- A: rows, masks and the automaton
    int bad = 0;
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad);
    if (tid < AV_MAX_STATES) {
        unsigned raw = 0, cl = 0;
        for (int c = 0; c < 4; ++c) {
            const unsigned nxt = tid < A ? a.delta[4 * tid + c] : AV_DEAD;
            const bool dead = nxt >= (unsigned)A || ((term >> (nxt & 63u)) & 1ull);
            raw |= (nxt & 255u) << (8 * c);
            cl |= (dead ? AV_DEAD : (unsigned)__popcll(~term & ((1ull << (nxt & 63u)) - 1ull))) << (8 * c);      // live states before it
        }
        nx[tid] = raw; col[tid] = cl;
    }
    __syncthreads();
    // ---- B: l_t(a), t = n-1 .. 0; one wave, lane = state; l_n = 0 is not stored
    if (tid < AV_MAX_STATES) {
        const bool live = tid < A && !((term >> tid) & 1ull);
        const unsigned cl = col[tid];
        const int mine = __popcll(~term & ((1ull << tid) - 1ull));
        int cc[4], ok = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned k = (cl >> (8 * c)) & 255u;
            ok |= (k != AV_DEAD ? 1 : 0) << c;
            cc[c] = k != AV_DEAD ? (int)k : 0;
        }
        for (int t = n - 1; t >= 0; --t) {
            if (live) {
                const double* next = tab + (size_t)(t + 1) * AL;
                double l[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) l[c] = t + 1 < n ? next[cc[c]] : 0.0;
                const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
                const double v[4] = {z01.x + l[0], z01.y + l[1], z23.x + l[2], z23.y + l[3]};
                tab[(size_t)t * AL + mine] = ds_lse<4>(v, (int)ms[t] & ok);
            }
            ds_wave_sync();
        }
    }
    __syncthreads();
    const bool miss = n > 0 && !(tab[0] > -INFINITY);               // state 0 is live and has column 0
    if (tid == 0 && a.miss) a.miss[b] = miss ? 1 : 0;
    // ---- C: the walks of 64 samples, then their rows
    const int S = (a.seqs || a.seq_nll || a.hits) ? a.S : 1;         // `infeasible` is written with sample 0
    for (int s0 = 0; s0 < S; s0 += AV_CHUNK) {
        const int cn = min(AV_CHUNK, S - s0);
        if (tid < cn) {
            const int s = s0 + tid;
            unsigned* mine = draws + tid * W;
            unsigned word = 0;
            int st = 0, hit = 0;
            for (int t = 0; t < n; ++t) {
                DsPos<double> p;
                const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
                p.z[0] = z01.x; p.z[1] = z01.y; p.z[2] = z23.x; p.z[3] = z23.y;
                p.m = ms[t];
                const unsigned u = ds_u24(seed, s, b, t);
                int q = -1;
                if (!miss) {
                    const unsigned cl = col[st];
                    const double* next = tab + (size_t)(t + 1) * AL;
                    double v[4];
                    int adm = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const unsigned k = (cl >> (8 * c)) & 255u;
                        const bool in = ((p.m >> c) & 1) && k != AV_DEAD;
                        const double l = !in ? -INFINITY : t + 1 < n ? next[in ? k : 0] : 0.0;
                        v[c] = p.z[c] + l;
                        adm |= (in && l > -INFINITY ? 1 : 0) << c;
                    }
                    if (adm) {
                        double w[4];
                        ds_weights(v, adm, w);
                        q = ds_select(w, adm, u);
                    }
                }
                if (q < 0) q = ds_draw_single(p, u);                // no sequence avoids the motifs: rnampnn_design's draw
                const unsigned nxt = (nx[st] >> (8 * q)) & 255u;
                const bool out = nxt >= (unsigned)A;
                hit += out || ((term >> (nxt & 63u)) & 1ull) ? 1 : 0;
                st = out ? 0 : (int)nxt;
                word |= (unsigned)q << (2 * (t & 15));
                if ((t & 15) == 15 || t == n - 1) { mine[t >> 4] = word; word = 0; }
            }
            hitc[tid] = hit;
        }
        __syncthreads();
        for (int i = 0; i < cn; ++i) {
            const int s = s0 + i;
            const unsigned* row = draws + i * W;
            ds_write_rows(a, s, b, n, row0, tid, s == 0 ? bad : 0, sc, [&](int t) { return (int)((row[t >> 4] >> (2 * (t & 15))) & 3u); }, DsNoSum{});
            if (tid == 0 && a.hits) a.hits[(size_t)s * a.B + b] = hitc[i];
            __syncthreads();                                        // the scratch is written again by the next sample
        }
    }
}

// the bytes of dynamic LDS, from (T, live states) alone: the formula include/rnampnn_hip.h gives
size_t av_lds_bytes(long long T, long long live) {
    return av_rows_bytes(T, live) + (size_t)AV_CHUNK * 4 * (size_t)av_words((int)T) + 2 * 4 * AV_MAX_STATES + 4 * AV_CHUNK + AV_LDS_SCRATCH;
}
}  // namespace

extern "C" int rnampnn_design_avoid(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                    float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                    const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                    const uint8_t* delta, int32_t n_states, uint64_t terminal, int8_t* seqs, float* seq_nll,
                                    int32_t* infeasible, int32_t* hits, int32_t* avoid_miss, void* stream) {
    AvArgs a{};
    const int rc = av_prepare("rnampnn_design_avoid", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble,
                              bias, bias_per_position, seqs, seq_nll, infeasible, delta, n_states, terminal, a, [] { return RNAMPNN_OK; });
    if (rc != RNAMPNN_OK) return rc;
    const size_t lds = av_lds_bytes(T, a.live);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_avoid: T = %d with %d live states needs %zu bytes of LDS for the table of partition "
                    "sums, the limit is %zu (T <= %lld at this automaton)", (int)T, a.live, lds, DS_LDS_MAX,
                    ds_max_T([&](long long t) { return av_lds_bytes(t, a.live); }));
    if (!seqs && !seq_nll && !infeasible && !hits && !avoid_miss) return RNAMPNN_OK;    // nothing asked for
    a.S = S; a.words = av_words(T); a.hits = hits; a.miss = avoid_miss;
    return ds_launch<k_design_avoid>(dim3(B), lds, stream, a);
}
