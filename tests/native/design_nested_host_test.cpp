// The host side of rnampnn_design_nested (rna-mpnn_amd/csrc/design_nested.hip) as a stand-alone program: the size formulas and every
// check that returns before a launch - the BAD_ARG cases, the workspace, the live-state limit, the LDS ceiling and "nothing asked for";
// a non-null partner passes them all.  It includes the translation unit itself (compiled for the host only), supplies the library's
// fail() and never reaches a launch, so it runs on a machine without a GPU; tests/test_design_nested_host_cpu.py builds it with the
// address and undefined-behaviour sanitizers.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "design_nested.hip"

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

static size_t lds_formula(size_t T, size_t L) {                    // include/rnampnn_hip.h's words
    const size_t tiles = 16 * L * L, draws = 1024 * (((T + 15) / 16) | 1);
    return 36 * T + (tiles > draws ? tiles : draws) + 1952;
}

int main() {
    // ---- the formulas
    EXPECT(rnampnn_design_nested_workspace_bytes(9, 300, 53) == (size_t)8 * 9 * 300 * 53 * 53 + (size_t)256 * 9 * 151);
    EXPECT(rnampnn_design_nested_workspace_bytes(1, 1, 1) == 8 + 256 && rnampnn_design_nested_workspace_bytes(1, 3, 2) == 96 + 512);
    EXPECT(rnampnn_design_nested_workspace_bytes(0, 300, 13) == 0 && rnampnn_design_nested_workspace_bytes(9, -1, 13) == 0 &&
           rnampnn_design_nested_workspace_bytes(9, 300, 0) == 0);
    EXPECT(rnampnn_design_nested_workspace_bytes(65536, 65536, 64) == (size_t)8 * 65536 * 65536 * 4096 + (size_t)256 * 65536 * 32769);   // past 2^32
    for (int L : {1, 13, 53, 64})
        for (int T : {1, 16, 17, 300, 1000, 1616, 1617}) EXPECT(ns_lds_bytes(T, L) == lds_formula(T, L));
    EXPECT(ns_lds_bytes(1000, 64) == 103488 && ns_lds_bytes(1000, 13) == 102464 && ns_lds_bytes(300, 13) == 32208 && ns_lds_bytes(300, 53) == 57696);
    EXPECT(ns_lds_bytes(1616, 64) == 163552 && ns_lds_bytes(1617, 64) == 165636);
    for (int L : {1, 13, 64}) EXPECT(ds_max_T([L](long long t) { return ns_lds_bytes(t, L); }) >= 1000);
    EXPECT(dfa_words(1) == 1 && dfa_words(16) == 1 && dfa_words(17) == 3 && dfa_words(1000) == 63);
    // ---- the checks; the "device" pointers are host memory that nothing dereferences before the call returns
    const int B = 2, T = 40, A = 5;
    alignas(16) static float logits[B * T * 4];
    static float mask[B * T];
    static int32_t cu[B + 1] = {0, 40, 80}, partner[B * T];
    static uint8_t delta[4 * 256];
    std::vector<uint8_t> kind(A, 2);
    kind[4] = 1;                                                   // 4 live states
    const size_t need = rnampnn_design_nested_workspace_bytes(B, T, 4);
    std::vector<double> ws(need / 8);
    static int8_t seqs[8 * B * T];
    auto call = [&](const float* lg, const float* m, const int32_t* c, int b, int t, float temp, int S, const uint8_t* d, const uint8_t* k, int n,
                    void* w, size_t wb, const int32_t* pa, bool outputs) {
        g_error[0] = 0;
        return rnampnn_design_nested(lg, (int64_t)B * T, m, c, b, t, temp, S, 1, nullptr, nullptr, pa, 1, nullptr, 0, d, k, n, w, wb,
                                     outputs ? seqs : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    const int BAD = RNAMPNN_ERR_BAD_ARG, UNS = RNAMPNN_ERR_UNSUPPORTED;
    EXPECT(need % 8 == 0);
    EXPECT(call(nullptr, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, 0, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, 0, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 0, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 65535, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, nullptr, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, cu, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 0.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits + 1, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, nullptr, kind.data(), A, ws.data(), need, nullptr, true) == BAD && std::strstr(g_error, "null delta"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, nullptr, A, ws.data(), need, nullptr, true) == BAD && std::strstr(g_error, "null kind"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), 0, ws.data(), need, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), 257, ws.data(), need, nullptr, true) == BAD && std::strstr(g_error, "1 .. 256"));
    std::vector<uint8_t> dead0(kind);
    dead0[0] = 3;
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, dead0.data(), A, ws.data(), need, nullptr, true) == BAD && std::strstr(g_error, "marked dead"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, nullptr, need, nullptr, true) == BAD && std::strstr(g_error, "is null"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need - 1, nullptr, true) == BAD && std::strstr(g_error, "too small"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), 0, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, (char*)ws.data() + 4, need, nullptr, true) == BAD && std::strstr(g_error, "aligned"));
    // more than 64 live states: UNSUPPORTED naming the count and the limit; a workspace of the right size comes first
    {
        std::vector<uint8_t> many(80, 2);
        for (int s = 73; s < 80; ++s) many[s] = 1;                  // 73 live
        std::vector<double> w3(rnampnn_design_nested_workspace_bytes(B, T, 73) / 8);
        EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, many.data(), 80, w3.data(), w3.size() * 8, nullptr, true) == UNS &&
               std::strstr(g_error, "73 live states") && std::strstr(g_error, "limit is 64"));
        EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, many.data(), 80, w3.data(), w3.size() * 8 - 8, nullptr, true) == BAD);
        std::vector<uint8_t> edge(80, 1);
        for (int s = 0; s < 64; ++s) edge[s] = 2;                   // exactly 64 live: accepted (nothing asked for, so no launch)
        std::vector<double> w4(rnampnn_design_nested_workspace_bytes(B, T, 64) / 8);
        EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, edge.data(), 80, w4.data(), w4.size() * 8, partner, false) == RNAMPNN_OK);
    }
    // the LDS ceiling is an UNSUPPORTED that names the bytes, the limit and the largest T
    {
        const int TT = 1617;
        std::vector<float> big((size_t)4 * TT), m1(TT, 1.f);
        std::vector<double> w1(rnampnn_design_nested_workspace_bytes(1, TT, 4) / 8);
        g_error[0] = 0;
        int rc = rnampnn_design_nested(big.data(), TT, m1.data(), nullptr, 1, TT, 1.f, 1, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, delta, kind.data(), A,
                                       w1.data(), w1.size() * 8, seqs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        EXPECT(rc == UNS && std::strstr(g_error, "165636") && std::strstr(g_error, "163840") && std::strstr(g_error, "T <= 1616"));
        rc = rnampnn_design_nested(big.data(), TT - 1, m1.data(), nullptr, 1, TT - 1, 1.f, 1, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, delta, kind.data(), A,
                                   w1.data(), w1.size() * 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        EXPECT(rc == RNAMPNN_OK);
    }
    // every output null: RNAMPNN_OK without a launch (a launch would need a device), with and without a partner table
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, false) == RNAMPNN_OK);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, partner, false) == RNAMPNN_OK);
    if (g_bad) return 1;
    std::printf("design_nested_host_test: ok\n");
    return 0;
}
