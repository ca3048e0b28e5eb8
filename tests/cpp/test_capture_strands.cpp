// GPU: the graph that eight captured cpi_preintegrate_batch calls leave behind on two STRANDS (include/cpi_amd.h:
// cpi_ctx_set_capture_strands), read back with hipGraphGetNodes / hipGraphGetEdges.  Product library only; the program checks
// itself and prints "test_capture_strands ok" as its last line.  Built and run by tests/test_gpu_capture_strands_cpp.py.
//   disjoint   eight calls into eight output sets: node i >= 2 has exactly one in-edge, from node i-2; no path either way between
//              i and i-1; 6 edges in all; after two replays the graph has written bit for bit what the eager calls write
//              (W = 640, N = 9 and W = 130, N = 50)
//   same       all calls into one output set: a chain of 7 edges
//   one row    call 5's DT array begins on the last row of call 4's: an edge 4 -> 5 and none 3 -> 5; call 6 goes to the other
//              strand, behind call 3
//   n = 1      a chain
//   memcpy     a hipMemcpyAsync captured after call 4: it has paths from nodes 0-4, nodes 5-7 have paths from it, nodes 5 and 6
//              both have an edge from it, node 7 follows node 5
// A process that sets GPU_MAX_HW_QUEUES below 4 keeps the serial shape: the program then expects chains everywhere.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <vector>

#include "../../include/cpi_amd.h"

static int g_fail = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
    } while (0)
#define HIP(call)                                                          \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) { printf("HIP error %s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); exit(2); } \
    } while (0)
#define CPI(call)                                                          \
    do {                                                                   \
        if ((call) != CPI_OK) { printf("cpi error %s:%d: %s: %s\n", __FILE__, __LINE__, #call, cpi_last_error(g_ctx)); exit(2); } \
    } while (0)

static cpi_ctx *g_ctx = nullptr;
static hipStream_t g_stream = nullptr;
constexpr int kCalls = 8, kMeanDoubles = 1 + 3 + 3 + 4;

struct Buffers {
    int64_t W;
    int32_t N;
    double *knots[2], *lin[2];       // two input batches
    double *out[kCalls + 1];         // mean output sets, kMeanDoubles * W doubles each (DT | alpha | beta | q)
    double *spare_lin;               // the memcpy scenario's source
};
static void make_inputs(Buffers &b) {
    const int64_t W = b.W;
    const int32_t N = b.N;
    for (int s = 0; s < 2; s++) {
        std::vector<double> kn((size_t)W * (N + 1) * 7), lin((size_t)W * 6);
        for (int64_t w = 0; w < W; w++) {
            for (int k = 0; k <= N; k++) {
                double *r = &kn[((size_t)w * (N + 1) + k) * 7];
                r[0] = 0.005 * k + 1e-3 * (double)w;
                for (int c = 0; c < 3; c++) {
                    r[1 + c] = 0.3 * std::sin(0.01 * (double)(w + 1) * (c + 1) + 0.2 * k + s);
                    r[4 + c] = (c == 2 ? 9.81 : 0.0) + 0.5 * std::cos(0.02 * (double)(w + 1) + 0.3 * k * (c + 1) + s);
                }
            }
            for (int c = 0; c < 6; c++) lin[(size_t)w * 6 + c] = 1e-3 * (c + 1) * (s + 1);
        }
        HIP(hipMalloc((void **)&b.knots[s], kn.size() * 8));
        HIP(hipMalloc((void **)&b.lin[s], lin.size() * 8));
        HIP(hipMemcpy(b.knots[s], kn.data(), kn.size() * 8, hipMemcpyHostToDevice));
        HIP(hipMemcpy(b.lin[s], lin.data(), lin.size() * 8, hipMemcpyHostToDevice));
    }
    for (int i = 0; i <= kCalls; i++) HIP(hipMalloc((void **)&b.out[i], (size_t)W * kMeanDoubles * 8));
    HIP(hipMalloc((void **)&b.spare_lin, (size_t)W * 6 * 8));
    HIP(hipMemcpy(b.spare_lin, b.lin[1], (size_t)W * 6 * 8, hipMemcpyDeviceToDevice));
}
static void free_inputs(Buffers &b) {
    for (int s = 0; s < 2; s++) { HIP(hipFree(b.knots[s])); HIP(hipFree(b.lin[s])); }
    for (int i = 0; i <= kCalls; i++) HIP(hipFree(b.out[i]));
    HIP(hipFree(b.spare_lin));
}
static cpi_outputs outputs_at(const Buffers &b, double *base) {
    cpi_outputs o;
    memset(&o, 0, sizeof o);
    o.DT = base; o.alpha = base + b.W; o.beta = base + 4 * b.W; o.q = base + 7 * b.W;
    return o;
}
static cpi_params params() {
    cpi_params p;
    memset(&p, 0, sizeof p);
    p.sigma_w = 1e-3; p.sigma_wb = 1e-5; p.sigma_a = 1e-2; p.sigma_ab = 1e-4;
    p.grav[2] = 9.81;
    p.model = CPI_MODEL_V1;
    p.state_transition_jacobians = 1;
    return p;
}

// A capture of kCalls calls; `out_of(i)` picks call i's outputs; memcpy_after >= 0: a copy into lin[1] captured after that call.
struct Captured {
    hipGraph_t graph = nullptr;
    std::vector<hipGraphNode_t> node;   // node[i]: call i's kernel node
    hipGraphNode_t copy = nullptr;
    std::vector<hipGraphNode_t> from, to;
    bool edge(hipGraphNode_t a, hipGraphNode_t b) const {
        for (size_t e = 0; e < from.size(); e++) if (from[e] == a && to[e] == b) return true;
        return false;
    }
    int in_edges(hipGraphNode_t b) const {
        int n = 0;
        for (size_t e = 0; e < to.size(); e++) n += to[e] == b;
        return n;
    }
    bool path(hipGraphNode_t a, hipGraphNode_t b) const {
        std::vector<hipGraphNode_t> todo(1, b), seen;
        while (!todo.empty()) {
            hipGraphNode_t n = todo.back();
            todo.pop_back();
            if (n == a) return true;
            bool was = false;
            for (hipGraphNode_t s : seen) was = was || s == n;
            if (was) continue;
            seen.push_back(n);
            for (size_t e = 0; e < to.size(); e++) if (to[e] == n) todo.push_back(from[e]);
        }
        return false;
    }
};
// the node the last call added: the one among the stream's capture dependencies that was not known before
static hipGraphNode_t new_node(std::vector<hipGraphNode_t> &known) {
    hipStreamCaptureStatus st;
    unsigned long long id = 0;
    const hipGraphNode_t *deps = nullptr;
    size_t nd = 0;
    HIP(hipStreamGetCaptureInfo_v2(g_stream, &st, &id, nullptr, &deps, &nd));
    CHECK(st == hipStreamCaptureStatusActive);
    hipGraphNode_t fresh = nullptr;
    int nfresh = 0;
    for (size_t i = 0; i < nd; i++) {
        bool was = false;
        for (hipGraphNode_t k : known) was = was || k == deps[i];
        if (!was) { fresh = deps[i]; nfresh++; }
    }
    CHECK(nfresh == 1);
    known.push_back(fresh);
    return fresh;
}
template <class OutOf>
static Captured capture(const Buffers &b, OutOf out_of, int memcpy_after) {
    Captured c;
    const cpi_params p = params();
    std::vector<hipGraphNode_t> known;
    HIP(hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kCalls; i++) {
        const cpi_outputs o = out_of(i);
        CPI(cpi_preintegrate_batch(g_ctx, &p, b.W, b.N, b.knots[i % 2], nullptr, nullptr, b.lin[i % 2], nullptr, &o));
        c.node.push_back(new_node(known));
        if (i == memcpy_after) {
            HIP(hipMemcpyAsync(b.lin[1], b.spare_lin, (size_t)b.W * 6 * 8, hipMemcpyDeviceToDevice, g_stream));
            c.copy = new_node(known);
        }
    }
    HIP(hipStreamEndCapture(g_stream, &c.graph));
    size_t nn = 0, ne = 0;
    HIP(hipGraphGetNodes(c.graph, nullptr, &nn));
    CHECK(nn == (size_t)kCalls + (memcpy_after >= 0 ? 1 : 0));
    HIP(hipGraphGetEdges(c.graph, nullptr, nullptr, &ne));
    c.from.resize(ne); c.to.resize(ne);
    if (ne) HIP(hipGraphGetEdges(c.graph, c.from.data(), c.to.data(), &ne));
    return c;
}
static void expect_chain(const Captured &c) {
    for (int i = 1; i < kCalls; i++) CHECK(c.edge(c.node[i - 1], c.node[i]));
    CHECK(c.from.size() == (size_t)kCalls - 1);
}
// two strands, all calls disjoint: call i behind call i - 2 and nothing else
static void expect_two_chains(const Captured &c) {
    CHECK(c.in_edges(c.node[0]) == 0 && c.in_edges(c.node[1]) == 0);
    for (int i = 2; i < kCalls; i++) CHECK(c.in_edges(c.node[i]) == 1 && c.edge(c.node[i - 2], c.node[i]));
    for (int i = 1; i < kCalls; i++) CHECK(!c.path(c.node[i - 1], c.node[i]) && !c.path(c.node[i], c.node[i - 1]));
    CHECK(c.from.size() == (size_t)kCalls - 2);
}

static void run_shape(int64_t W, int32_t N, int S, bool all_scenarios) {
    Buffers b;
    b.W = W; b.N = N;
    make_inputs(b);
    const cpi_params p = params();
    const size_t out_bytes = (size_t)W * kMeanDoubles * 8;

    // disjoint: eager reference first, then the graph's outputs against it, bit for bit
    std::vector<std::vector<double>> ref(kCalls, std::vector<double>((size_t)W * kMeanDoubles)), got = ref;
    for (int i = 0; i < kCalls; i++) {
        const cpi_outputs o = outputs_at(b, b.out[i]);
        CPI(cpi_preintegrate_batch(g_ctx, &p, W, N, b.knots[i % 2], nullptr, nullptr, b.lin[i % 2], nullptr, &o));
    }
    HIP(hipStreamSynchronize(g_stream));
    for (int i = 0; i < kCalls; i++) {
        HIP(hipMemcpy(ref[i].data(), b.out[i], out_bytes, hipMemcpyDeviceToHost));
        HIP(hipMemset(b.out[i], 0xff, out_bytes));
    }
    {
        Captured c = capture(b, [&](int i) { return outputs_at(b, b.out[i]); }, -1);
        if (S > 1) expect_two_chains(c); else expect_chain(c);
        hipGraphExec_t exec = nullptr;
        HIP(hipGraphInstantiate(&exec, c.graph, nullptr, nullptr, 0));
        for (int rep = 0; rep < 2; rep++) HIP(hipGraphLaunch(exec, g_stream));
        HIP(hipStreamSynchronize(g_stream));
        for (int i = 0; i < kCalls; i++) {
            HIP(hipMemcpy(got[i].data(), b.out[i], out_bytes, hipMemcpyDeviceToHost));
            CHECK(memcmp(got[i].data(), ref[i].data(), out_bytes) == 0);
        }
        HIP(hipGraphExecDestroy(exec));
        HIP(hipGraphDestroy(c.graph));
    }
    if (all_scenarios) {
        {   // every call writes the same output set
            Captured c = capture(b, [&](int) { return outputs_at(b, b.out[0]); }, -1);
            expect_chain(c);
            HIP(hipGraphDestroy(c.graph));
        }
        {   // call 5's DT array begins at the last row of call 4's
            Captured c = capture(b, [&](int i) {
                cpi_outputs o = outputs_at(b, b.out[i]);
                if (i == 5) { o = outputs_at(b, b.out[kCalls]); o.DT = b.out[4] + (W - 1); }
                if (i == 4) { o.alpha = nullptr; o.beta = nullptr; o.q = nullptr; }   // (call 5's DT runs into what would be call 4's alpha)
                return o; }, -1);
            if (S > 1) {   // 0 2 4 5 7 on one strand, 1 3 6 on the other
                CHECK(c.edge(c.node[4], c.node[5]) && !c.edge(c.node[3], c.node[5]) && c.in_edges(c.node[5]) == 1);
                CHECK(c.edge(c.node[3], c.node[6]) && c.in_edges(c.node[6]) == 1 && !c.path(c.node[5], c.node[6]) && !c.path(c.node[4], c.node[6]));
                CHECK(c.edge(c.node[5], c.node[7]) && c.in_edges(c.node[7]) == 1);
                for (int i = 2; i <= 4; i++) CHECK(c.in_edges(c.node[i]) == 1 && c.edge(c.node[i - 2], c.node[i]));
                CHECK(c.from.size() == (size_t)kCalls - 2);
            } else expect_chain(c);
            HIP(hipGraphDestroy(c.graph));
        }
        {   // one strand
            CPI(cpi_ctx_set_capture_strands(g_ctx, 1));
            Captured c = capture(b, [&](int i) { return outputs_at(b, b.out[i]); }, -1);
            expect_chain(c);
            HIP(hipGraphDestroy(c.graph));
            CPI(cpi_ctx_set_capture_strands(g_ctx, 2));
        }
        {   // the caller's own copy between calls 4 and 5
            Captured c = capture(b, [&](int i) { return outputs_at(b, b.out[i]); }, 4);
            for (int i = 0; i <= 4; i++) CHECK(c.path(c.node[i], c.copy));
            for (int i = 5; i < kCalls; i++) CHECK(c.path(c.copy, c.node[i]));
            if (S > 1) {   // the copy joins both strands (3 and 4 are its predecessors); a fresh window behind it: 5 and 6 hang off it, 7 follows 5
                CHECK(c.edge(c.node[3], c.copy) && c.edge(c.node[4], c.copy) && c.in_edges(c.copy) == 2);
                CHECK(c.edge(c.copy, c.node[5]) && c.edge(c.copy, c.node[6]) && c.in_edges(c.node[5]) == 1 && c.in_edges(c.node[6]) == 1);
                CHECK(c.edge(c.node[5], c.node[7]) && c.in_edges(c.node[7]) == 1);
                CHECK(!c.path(c.node[5], c.node[6]) && !c.path(c.node[6], c.node[7]));
            }
            HIP(hipGraphDestroy(c.graph));
        }
    }
    free_inputs(b);
}

int main() {
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    const int S = (q && *q && atoi(q) < 4) ? 1 : 2;
    HIP(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    if (cpi_ctx_create(-1, g_stream, &g_ctx) != CPI_OK) { printf("cpi_ctx_create: %s\n", cpi_last_error(nullptr)); return 2; }
    CPI(cpi_ctx_set_capture_strands(g_ctx, 2));
    run_shape(640, 9, S, true);
    run_shape(130, 50, S, false);
    cpi_ctx_destroy(g_ctx);
    HIP(hipStreamDestroy(g_stream));
    if (g_fail) { printf("test_capture_strands: %d checks FAILED\n", g_fail); return 1; }
    printf("test_capture_strands ok (%d strands)\n", S);
    return 0;
}
