// The host side of rnampnn_design_dfa_count (rna-mpnn_amd/csrc/design_dfa_count.hip) as a stand-alone program: the size formulas and every
// check that returns before a launch - the BAD_ARG cases of the automaton, the count side and the workspace, the partner refusal, the LDS
// ceiling and "nothing asked for".  It includes the translation unit itself (compiled for the host only), supplies the library's fail()
// and never reaches a launch, so it runs on a machine without a GPU; tests/test_design_dfa_count_host_cpu.py builds it with the address
// and undefined-behaviour sanitizers.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "design_dfa_count.hip"

static char g_error[1024];
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

static int g_bad = 0;
#define EXPECT(cond)                                                                                     \
    do {                                                                                                 \
        if (!(cond)) { std::printf("line %d: %s (last error: %s)\n", __LINE__, #cond, g_error); ++g_bad; } \
    } while (0)

int main() {
    // ---- the formulas
    EXPECT(rnampnn_design_dfa_count_workspace_bytes(9, 72, 73, 8) == (size_t)8 * 9 * 72 * 73 * 9);
    EXPECT(rnampnn_design_dfa_count_workspace_bytes(9, 72, 73, 100000) == (size_t)8 * 9 * 72 * 73 * 73);     // cap = min(count_cap, T)
    EXPECT(rnampnn_design_dfa_count_workspace_bytes(256, 140, 13, 8) == 33546240 && rnampnn_design_dfa_count_workspace_bytes(256, 140, 13, 140) == 525557760);
    EXPECT(rnampnn_design_dfa_count_workspace_bytes(0, 72, 73, 8) == 0 && rnampnn_design_dfa_count_workspace_bytes(9, -1, 73, 8) == 0 &&
           rnampnn_design_dfa_count_workspace_bytes(9, 72, 0, 8) == 0 && rnampnn_design_dfa_count_workspace_bytes(9, 72, 73, 0) == 0);
    EXPECT(rnampnn_design_dfa_count_workspace_bytes(65536, 65536, 256, 65536) == (size_t)8 * 65536 * 65536 * 256 * 65537);    // size_t arithmetic
    EXPECT(dfc_table_bytes(9, 72, 73, 0) == (size_t)8 * 9 * 72 * 73);                                       // cap 0: one slab per position
    EXPECT(dfc_lds_bytes(72) == 11776 && dfc_lds_bytes(300) == 33856 && dfc_lds_bytes(1616) == 162560 && dfc_lds_bytes(1617) == 164672);
    EXPECT(ds_max_T([](long long t) { return dfc_lds_bytes(t); }) == 1616);
    EXPECT(dfc_slab_bytes(13, 8) == 1872 && dfc_slab_bytes(73, 72) == 85264 && dfc_slab_bytes(256, 72) == 299008);
    EXPECT(dfa_words(1) == 1 && dfa_words(16) == 1 && dfa_words(17) == 3 && dfa_words(1616) == 101);
    // ---- the checks; the "device" pointers are host memory that nothing dereferences before the call returns
    const int B = 2, T = 40, A = 5, CAP = 6;
    alignas(16) static float logits[B * T * 4];
    static float mask[B * T];
    static int32_t cu[B + 1] = {0, 40, 80}, partner[B * T], lo[B], hi[B] = {6, 6};
    static uint8_t delta[4 * 256], counted[B * T];
    std::vector<uint8_t> kind(A, 2);
    kind[4] = 1;                                                   // 4 live states
    const size_t need = rnampnn_design_dfa_count_workspace_bytes(B, T, 4, CAP);
    EXPECT(need == (size_t)8 * B * T * 4 * (CAP + 1));
    std::vector<double> ws(need / 8);
    static int8_t seqs[8 * B * T];
    struct Call {
        const float* lg = logits; const float* m = mask; const int32_t* c = nullptr; int b = B, t = T; float temp = 1.f; int S = 8;
        const uint8_t* d = delta; const uint8_t* k = nullptr; int n = A; const uint8_t* cs = counted; const int32_t* l = lo; const int32_t* h = hi;
        int cap = CAP; void* w = nullptr; size_t wb = 0; const int32_t* pa = nullptr; bool outputs = true;
    };
    auto call = [&](Call x) {
        g_error[0] = 0;
        return rnampnn_design_dfa_count(x.lg, (int64_t)B * T, x.m, x.c, x.b, x.t, x.temp, x.S, 1, nullptr, nullptr, x.pa, 1, nullptr, 0, x.d, x.k, x.n,
                                        x.cs, x.l, x.h, x.cap, x.w, x.wb, x.outputs ? seqs : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
    };
    Call ok;
    ok.k = kind.data(); ok.w = ws.data(); ok.wb = need;
    const int BAD = RNAMPNN_ERR_BAD_ARG, UNS = RNAMPNN_ERR_UNSUPPORTED;
    { Call x = ok; x.lg = nullptr; EXPECT(call(x) == BAD); }
    { Call x = ok; x.b = 0; EXPECT(call(x) == BAD); }
    { Call x = ok; x.t = 0; EXPECT(call(x) == BAD); }
    { Call x = ok; x.S = 0; EXPECT(call(x) == BAD); }
    { Call x = ok; x.S = 65535; EXPECT(call(x) == BAD); }
    { Call x = ok; x.m = nullptr; EXPECT(call(x) == BAD); }
    { Call x = ok; x.c = cu; EXPECT(call(x) == BAD); }
    { Call x = ok; x.temp = 0.f; EXPECT(call(x) == BAD); }
    { Call x = ok; x.lg = logits + 1; EXPECT(call(x) == BAD); }
    { Call x = ok; x.d = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "null delta")); }
    { Call x = ok; x.k = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "null kind")); }
    { Call x = ok; x.n = 0; EXPECT(call(x) == BAD); }
    { Call x = ok; x.n = 257; EXPECT(call(x) == BAD && std::strstr(g_error, "1 .. 256")); }
    std::vector<uint8_t> dead0(kind);
    dead0[0] = 3;
    { Call x = ok; x.k = dead0.data(); EXPECT(call(x) == BAD && std::strstr(g_error, "marked dead")); }
    { Call x = ok; x.cs = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "null counted, count_lo or count_hi")); }
    { Call x = ok; x.l = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "null counted, count_lo or count_hi")); }
    { Call x = ok; x.h = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "null counted, count_lo or count_hi")); }
    { Call x = ok; x.cap = -1; EXPECT(call(x) == BAD && std::strstr(g_error, "is negative")); }
    { Call x = ok; x.w = nullptr; EXPECT(call(x) == BAD && std::strstr(g_error, "is null") && std::strstr(g_error, "needs 17920")); }
    { Call x = ok; x.wb = need - 1; EXPECT(call(x) == BAD && std::strstr(g_error, "too small") && std::strstr(g_error, "needs 17920")); }
    { Call x = ok; x.wb = 0; EXPECT(call(x) == BAD); }
    { Call x = ok; x.w = (char*)ws.data() + 4; EXPECT(call(x) == BAD && std::strstr(g_error, "aligned")); }
    { Call x = ok; x.cap = CAP + 1; EXPECT(call(x) == BAD && std::strstr(g_error, "too small")); }         // the table grows with the cap
    { Call x = ok; x.cap = 0; x.wb = (size_t)8 * B * T * 4; x.outputs = false; EXPECT(call(x) == RNAMPNN_OK); x.wb -= 8; EXPECT(call(x) == BAD); }   // cap 0: one slab
    { Call x = ok; x.pa = partner; EXPECT(call(x) == UNS && std::strstr(g_error, "4^depth")); }
    // the LDS ceiling is an UNSUPPORTED that names the bytes, the limit and the largest T; a workspace of the right size comes first
    {
        const int TT = 1617;
        std::vector<float> big((size_t)4 * TT), m1(TT, 1.f);
        std::vector<uint8_t> c1(TT);
        std::vector<double> w1(rnampnn_design_dfa_count_workspace_bytes(1, TT, 4, 2) / 8);
        g_error[0] = 0;
        const int rc = rnampnn_design_dfa_count(big.data(), TT, m1.data(), nullptr, 1, TT, 1.f, 1, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, delta,
                                                kind.data(), A, c1.data(), lo, hi, 2, w1.data(), w1.size() * 8, seqs, nullptr, nullptr, nullptr, nullptr,
                                                nullptr, nullptr, nullptr, nullptr, nullptr);
        EXPECT(rc == UNS && std::strstr(g_error, "164672") && std::strstr(g_error, "163840") && std::strstr(g_error, "T <= 1616"));
    }
    // every output null: RNAMPNN_OK without a launch (a launch would need a device)
    { Call x = ok; x.outputs = false; EXPECT(call(x) == RNAMPNN_OK); }
    // a kind array of exactly n_states bytes and a full 256-state automaton: the host loops stay inside it (the sanitizer watches)
    std::vector<uint8_t> full(256, 2);
    std::vector<double> w2(rnampnn_design_dfa_count_workspace_bytes(B, T, 256, CAP) / 8);
    { Call x = ok; x.k = full.data(); x.n = 256; x.w = w2.data(); x.wb = w2.size() * 8; x.outputs = false; EXPECT(call(x) == RNAMPNN_OK); }
    { Call x = ok; x.k = full.data(); x.n = 256; x.w = w2.data(); x.wb = w2.size() * 8 - 8; x.outputs = false; EXPECT(call(x) == BAD); }
    if (g_bad) return 1;
    std::printf("design_dfa_count_host_test: ok\n");
    return 0;
}
