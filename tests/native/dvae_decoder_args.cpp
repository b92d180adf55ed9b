// The table of bad D-VAE decoder arguments of tests/test_dvae_decoder_args_cpu.py, run from C against the built library:
// for both entry points (dagnn_dvae_decode_forward / _backward, dagnn_dvae_sample) and both struct generations, every
// row makes the size queries return 0 and the entry point DAGNN_EINVAL, and every missing weight pointer DAGNN_EINVAL.
// Nothing is launched: workspace sizes are 0, so arguments that pass every check stop at DAGNN_ENOSPC - which the
// untouched baseline must, or a row would prove nothing.
//
// The earlier struct generation (no key_type behind mapper_w) is placed so that it ENDS at a page without access
// rights: a read behind it - key_type looked at before `agg` and `bn` admit it - ends the program with a fault, whether
// or not the library itself was built with a sanitizer.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tests/native/dvae_decoder_args.cpp -Ldagnn_amd/lib -ldagnn_hip -Wl,-rpath,$PWD/dagnn_amd/lib -o dvae_decoder_args
// (or any C++17 compiler, with the HIP runtime's library on the link line).  Prints the rows that fail; exit 0 if none.
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

#include "../../include/dagnn_hip.h"

static float dummy[64];   // what every pointer of a baseline points at; never dereferenced
static int failures = 0;

static void expect(bool ok, const char* entry, const char* gen, const char* what, const char* want) {
    if (ok) return;
    ++failures;
    printf("FAIL %s (%s struct): %s: expected %s\n", entry, gen, what, want);
}

template <typename A> struct Row {
    const char* what;
    void (*set)(A&);
    bool typed;   // touches key_type, or needs it looked at: not for the earlier struct
};

// one table for both structs: they name the decoder's fields alike
template <typename A> static std::vector<Row<A>> bad_rows() {
    return {
        {"n = 1", [](A& a) { a.n = 1; }, false},
        {"n = MAX_N + 1", [](A& a) { a.n = DAGNN_DVAE_MAX_N + 1; }, false},
        {"hs = 0", [](A& a) { a.hs = 0; }, false},
        {"L = 0", [](A& a) { a.L = 0; }, false},
        {"L = MAX_STACKED + 1", [](A& a) { a.L = DAGNN_MAX_STACKED + 1; }, false},
        {"nvt = 0", [](A& a) { a.nvt = 0; }, false},
        {"nvt = MAX_TYPES + 1", [](A& a) { a.nvt = DAGNN_DVAE_MAX_TYPES + 1; }, false},
        {"start_type = -1", [](A& a) { a.start_type = -1; }, false},
        {"start_type = nvt", [](A& a) { a.start_type = a.nvt; }, false},
        {"bn = -1", [](A& a) { a.bn = -1; }, false},
        {"bn = 2", [](A& a) { a.bn = 2; }, false},
        {"edge_hidden = 0", [](A& a) { a.edge_hidden = 0; }, false},
        {"vertex_hidden = 0", [](A& a) { a.vertex_hidden = 0; }, false},
        {"agg = -1", [](A& a) { a.agg = -1; }, false},
        {"agg = 3", [](A& a) { a.agg = DAGNN_DVAE_AGG_ATTN_X + 1; }, false},
        {"gated_sum with bn = 1", [](A& a) { a.agg = DAGNN_DVAE_AGG_GATED_SUM; a.bn = 1; }, false},
        {"gated_sum without gate_w", [](A& a) { a.agg = DAGNN_DVAE_AGG_GATED_SUM; a.gate_w = nullptr; }, false},
        {"gated_sum without gate_b", [](A& a) { a.agg = DAGNN_DVAE_AGG_GATED_SUM; a.gate_b = nullptr; }, false},
        {"gated_sum without mapper_w", [](A& a) { a.agg = DAGNN_DVAE_AGG_GATED_SUM; a.mapper_w = nullptr; }, false},
        {"attn_x with bn = 0", [](A& a) { a.agg = DAGNN_DVAE_AGG_ATTN_X; a.bn = 0; }, false},
        {"attn_x without key_type", [](A& a) { a.agg = DAGNN_DVAE_AGG_ATTN_X; a.bn = 1; a.key_type = nullptr; }, true},
    };
}

template <typename A> static std::vector<Row<A>> weight_rows() {
    std::vector<Row<A>> rows = {
        {"h0", [](A& a) { a.h0 = nullptr; }, false},       {"w_key", [](A& a) { a.w_key = nullptr; }, false},
        {"av_w1", [](A& a) { a.av_w1 = nullptr; }, false}, {"av_b1", [](A& a) { a.av_b1 = nullptr; }, false},
        {"av_w2", [](A& a) { a.av_w2 = nullptr; }, false}, {"av_b2", [](A& a) { a.av_b2 = nullptr; }, false},
        {"ae_w1", [](A& a) { a.ae_w1 = nullptr; }, false}, {"ae_b1", [](A& a) { a.ae_b1 = nullptr; }, false},
        {"ae_w2", [](A& a) { a.ae_w2 = nullptr; }, false}, {"ae_b2", [](A& a) { a.ae_b2 = nullptr; }, false},
        {"w_ih[0]", [](A& a) { a.w_ih[0] = nullptr; }, false}, {"w_ih[1]", [](A& a) { a.w_ih[1] = nullptr; }, false},
        {"w_hh[0]", [](A& a) { a.w_hh[0] = nullptr; }, false}, {"w_hh[1]", [](A& a) { a.w_hh[1] = nullptr; }, false},
        {"b_ih[0]", [](A& a) { a.b_ih[0] = nullptr; }, false}, {"b_ih[1]", [](A& a) { a.b_ih[1] = nullptr; }, false},
        {"b_hh[0]", [](A& a) { a.b_hh[0] = nullptr; }, false}, {"b_hh[1]", [](A& a) { a.b_hh[1] = nullptr; }, false},
    };
    return rows;
}

// the decoder fields both structs share: NA attn_h, L = 2, every pointer set
template <typename A> static void fill_decoder(A& a) {
    memset(&a, 0, sizeof(a));
    a.B = 4; a.n = 8; a.hs = 6; a.L = 2; a.nvt = 5; a.start_type = 0; a.bn = 0; a.edge_hidden = 16; a.vertex_hidden = 32;
    a.agg = DAGNN_DVAE_AGG_ATTN_H;
    a.h0 = a.w_key = a.vid_bias = a.av_w1 = a.av_b1 = a.av_w2 = a.av_b2 = a.ae_w1 = a.ae_b1 = a.ae_w2 = a.ae_b2 = dummy;
    a.gate_w = a.gate_b = a.mapper_w = a.key_type = dummy;
    for (int l = 0; l < a.L; ++l) a.w_ih[l] = a.w_hh[l] = a.b_ih[l] = a.b_hh[l] = dummy;
}

static dagnn_dvae_decode_grads grads;

static dagnn_dvae_decode_args decode_baseline() {
    dagnn_dvae_decode_args a;
    fill_decoder(a);
    a.types = (const int32_t*)dummy; a.preds = (const uint32_t*)dummy; a.ll = dummy; a.saved = dummy; a.saved_bytes = 0;
    float** g = (float**)&grads.d_h0;   // every gradient pointer from d_h0 to the struct's end
    for (size_t i = 0; i < (sizeof(grads) - offsetof(dagnn_dvae_decode_grads, d_h0)) / sizeof(float*); ++i) g[i] = dummy;
    grads.g_res = dummy; grads.work = dummy; grads.work_bytes = 0;
    return a;
}

static dagnn_dvae_sample_args sample_baseline() {
    dagnn_dvae_sample_args a;
    fill_decoder(a);
    a.G = 2; a.end_type = 1; a.stochastic = 1;
    a.u_type = a.u_edge = dummy;
    a.types = (int32_t*)dummy; a.preds = (uint32_t*)dummy; a.nv = (int32_t*)dummy; a.work = dummy; a.work_bytes = 0;
    return a;
}

static bool queries_zero(const dagnn_dvae_decode_args* a) {
    return dagnn_dvae_decode_saved_bytes(a) == 0 && dagnn_dvae_decode_work_bytes(a) == 0;
}
static bool queries_positive(const dagnn_dvae_decode_args* a) {
    return dagnn_dvae_decode_saved_bytes(a) > 0 && dagnn_dvae_decode_work_bytes(a) > 0;
}
static bool entry_returns(const dagnn_dvae_decode_args* a, int rc) {
    return dagnn_dvae_decode_forward(a, nullptr) == rc && dagnn_dvae_decode_backward(a, &grads, nullptr) == rc;
}
static bool queries_zero(const dagnn_dvae_sample_args* a) { return dagnn_dvae_sample_work_bytes(a) == 0; }
static bool queries_positive(const dagnn_dvae_sample_args* a) { return dagnn_dvae_sample_work_bytes(a) > 0; }
static bool entry_returns(const dagnn_dvae_sample_args* a, int rc) { return dagnn_dvae_sample(a, nullptr) == rc; }

// a copy of the first `bytes` bytes of `a` that ends where a page without access rights begins
template <typename A> static const A* before_guard_page(const A& a, size_t bytes) {
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    char* p = (char*)mmap(nullptr, 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED || mprotect(p + page, page, PROT_NONE) != 0) {
        perror("guard page");
        _exit(2);
    }
    memcpy(p + page - bytes, &a, bytes);
    return (const A*)(p + page - bytes);
}

template <typename A> static void run(const char* entry, A (*baseline)()) {
    for (int typed = 0; typed < 2; ++typed) {
        const char* gen = typed ? "current" : "earlier";
        const size_t bytes = typed ? sizeof(A) : offsetof(A, key_type);
        auto check = [&](const Row<A>& r, bool is_bad) {
            if (r.typed && !typed) return;
            A a = baseline();
            r.set(a);
            const A* p = before_guard_page(a, bytes);
            if (is_bad) expect(queries_zero(p), entry, gen, r.what, "size queries 0");
            else expect(queries_positive(p), entry, gen, r.what, "size queries > 0 (a missing pointer is the entry point's to refuse)");
            expect(entry_returns(p, DAGNN_EINVAL), entry, gen, r.what, "DAGNN_EINVAL");
        };
        const A good = baseline();
        const A* p = before_guard_page(good, bytes);
        expect(queries_positive(p), entry, gen, "baseline", "size queries > 0");
        expect(entry_returns(p, DAGNN_ENOSPC), entry, gen, "baseline", "DAGNN_ENOSPC (every check passed, no workspace)");
        for (const Row<A>& r : bad_rows<A>()) check(r, true);
        for (const Row<A>& r : weight_rows<A>()) check(r, false);
    }
}

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);   // (a fault must not swallow the rows already reported)
    run<dagnn_dvae_decode_args>("dagnn_dvae_decode", decode_baseline);
    run<dagnn_dvae_sample_args>("dagnn_dvae_sample", sample_baseline);
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
