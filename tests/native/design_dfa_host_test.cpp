// The host side of rnampnn_design_dfa (rna-mpnn_amd/csrc/design_dfa.hip) as a stand-alone program: the size formulas and every check
// that returns before a launch - the BAD_ARG cases, the workspace, the partner refusal, the LDS ceiling and "nothing asked for" - and
// what dfa_chain_dev.h's dfa_prepare leaves in the automaton's arguments for the three entries that share it (live, dead[], acc[]).  It
// includes the translation unit itself (compiled for the host only), supplies the library's fail() and never reaches a launch, so it
// runs on a machine without a GPU; tests/test_design_dfa_host_cpu.py builds it with the address and undefined-behaviour sanitizers.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "design_dfa.hip"

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
    EXPECT(rnampnn_design_dfa_workspace_bytes(9, 300, 73) == (size_t)8 * 9 * 300 * 73);
    EXPECT(rnampnn_design_dfa_workspace_bytes(0, 300, 73) == 0 && rnampnn_design_dfa_workspace_bytes(9, -1, 73) == 0 &&
           rnampnn_design_dfa_workspace_bytes(9, 300, 0) == 0);
    EXPECT(rnampnn_design_dfa_workspace_bytes(65536, 65536, 256) == (size_t)8 * 65536 * 65536 * 256);      // past 2^32: size_t arithmetic
    EXPECT(dfa_lds_bytes(300) == 37392 && dfa_lds_bytes(1200) == 124432 && dfa_lds_bytes(1587) == 163840 && dfa_lds_bytes(1588) == 163872);
    EXPECT(ds_max_T([](long long t) { return dfa_lds_bytes(t); }) == 1587);
    EXPECT(dfa_words(1) == 1 && dfa_words(16) == 1 && dfa_words(17) == 3 && dfa_words(1587) == 101);
    // ---- the checks; the "device" pointers are host memory that nothing dereferences before the call returns
    const int B = 2, T = 40, A = 5;
    alignas(16) static float logits[B * T * 4];
    static float mask[B * T];
    static int32_t cu[B + 1] = {0, 40, 80}, partner[B * T];
    static uint8_t delta[4 * 256];
    std::vector<uint8_t> kind(A, 2);
    kind[4] = 1;                                                   // 4 live states
    const size_t need = rnampnn_design_dfa_workspace_bytes(B, T, 4);
    std::vector<double> ws(need / 8);
    static int8_t seqs[8 * B * T];
    auto call = [&](const float* lg, const float* m, const int32_t* c, int b, int t, float temp, int S, const uint8_t* d, const uint8_t* k, int n,
                    void* w, size_t wb, const int32_t* pa, bool outputs) {
        g_error[0] = 0;
        return rnampnn_design_dfa(lg, (int64_t)B * T, m, c, b, t, temp, S, 1, nullptr, nullptr, pa, 1, nullptr, 0, d, k, n, w, wb,
                                  outputs ? seqs : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    const int BAD = RNAMPNN_ERR_BAD_ARG, UNS = RNAMPNN_ERR_UNSUPPORTED;
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
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need - 1, nullptr, true) == BAD && std::strstr(g_error, "too small") &&
           std::strstr(g_error, "rnampnn_design_dfa: the workspace is too small (2559 bytes), the table of partition sums at (B = 2, T = 40, 4 live states) "
                                "needs 2560 (rnampnn_design_dfa_workspace_bytes)"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), 0, nullptr, true) == BAD);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, (char*)ws.data() + 4, need, nullptr, true) == BAD && std::strstr(g_error, "aligned"));
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, partner, true) == UNS && std::strstr(g_error, "4^depth"));
    // the LDS ceiling is an UNSUPPORTED that names the bytes, the limit and the largest T; a workspace of the right size comes first
    {
        const int TT = 1588;
        std::vector<float> big((size_t)4 * TT), m1(TT, 1.f);
        std::vector<double> w1(rnampnn_design_dfa_workspace_bytes(1, TT, 4) / 8);
        g_error[0] = 0;
        const int rc = rnampnn_design_dfa(big.data(), TT, m1.data(), nullptr, 1, TT, 1.f, 1, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, delta, kind.data(), A,
                                          w1.data(), w1.size() * 8, seqs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        EXPECT(rc == UNS && std::strstr(g_error, "163872") && std::strstr(g_error, "163840") && std::strstr(g_error, "T <= 1587"));
    }
    // every output null: RNAMPNN_OK without a launch (a launch would need a device)
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, kind.data(), A, ws.data(), need, nullptr, false) == RNAMPNN_OK);
    // a kind array of exactly n_states bytes and a full 256-state automaton: the host loops stay inside it (the sanitizer watches)
    std::vector<uint8_t> full(256, 2);
    std::vector<double> w2(rnampnn_design_dfa_workspace_bytes(B, T, 256) / 8);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, full.data(), 256, w2.data(), w2.size() * 8, nullptr, false) == RNAMPNN_OK);
    EXPECT(call(logits, mask, nullptr, B, T, 1.f, 8, delta, full.data(), 256, w2.data(), w2.size() * 8 - 8, nullptr, false) == BAD);
    // ---- the shared prologue (dfa_prepare): `kind` is read once - the count the workspace check is given is the `live` the kernel gets -
    // and dead[] / acc[] hold a bit per state in all four 64-bit words: 193 states, dead at 63, 127 and 191, accepting at 5, 64 and 192
    {
        const int N = 193;
        std::vector<uint8_t> wide(N, 0);
        wide[63] = wide[127] = 1;
        wide[191] = 3;                                              // dead wins over accepting
        wide[5] = wide[64] = wide[192] = 2;
        std::vector<double> w5(rnampnn_design_dfa_workspace_bytes(B, T, N) / 8);
        DfaArgs a{};
        int asked = 0, told = -1;
        g_error[0] = 0;
        const int rc = dfa_prepare("shared", logits, (int64_t)B * T, mask, nullptr, B, T, 1.f, 8, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, seqs, nullptr,
                                   nullptr, delta, wide.data(), N, w5.data(), w5.size() * 8, nullptr, nullptr, nullptr, true, a,
                                   [] { return RNAMPNN_OK; }, [&](int live, char* what, size_t len) {
            ++asked;
            told = live;
            std::snprintf(what, len, "the test's table needs");
            return rnampnn_design_dfa_workspace_bytes(B, T, live);
        });
        EXPECT(rc == RNAMPNN_OK && asked == 1 && told == 190 && a.live == 190 && a.A == N && a.S == 8 && a.words == dfa_words(T));
        EXPECT(a.dead[0] == 1ull << 63 && a.dead[1] == 1ull << 63 && a.dead[2] == 1ull << 63 && a.dead[3] == ~1ull);
        EXPECT(a.acc[0] == 1ull << 5 && a.acc[1] == 1ull && a.acc[2] == 0 && a.acc[3] == 1ull);
        EXPECT(a.delta == delta && a.tab == w5.data() && !a.hits && !a.accepted && !a.dfa_miss && a.seqs == seqs);
        // one byte short of what `live` states need: the message is built from the entry's words, the count and the name
        const int rc2 = dfa_prepare("shared", logits, (int64_t)B * T, mask, nullptr, B, T, 1.f, 8, 1, nullptr, nullptr, nullptr, 1, nullptr, 0, seqs,
                                    nullptr, nullptr, delta, wide.data(), N, w5.data(), (size_t)8 * B * T * 190 - 1, nullptr, nullptr, nullptr, true, a,
                                    [] { return RNAMPNN_OK; }, [&](int live, char* what, size_t len) {
            std::snprintf(what, len, "the test's table at %d live states needs", live);
            return rnampnn_design_dfa_workspace_bytes(B, T, live);
        });
        EXPECT(rc2 == BAD && std::strstr(g_error, "shared: the workspace is too small (121599 bytes), the test's table at 190 live states needs 121600 "
                                                  "(shared_workspace_bytes)"));
    }
    if (g_bad) return 1;
    std::printf("design_dfa_host_test: ok\n");
    return 0;
}
