// C-ABI entry points of liblinna_hip.so (declared in include/linna_hip.h) and the host-side
// orchestration above the kernels: network forward/backward as chains of fused GEMMs, the
// serving pipeline (Log_prob), the training loss, the ensemble moves.  No device allocation, no sync.  A subsystem with a
// file of its own keeps its entries there: hmc.hip, autocorr.hip, chain_rank.hip, comm.hip.
#include "common.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <cstring>
#include <string>
#include <vector>
#include <atomic>
#include <new>
#include <stdlib.h>

namespace linna {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int caught_exception(const char* what) noexcept {
    // (the text is built in a fixed buffer; if even the assignment cannot allocate, the previous text stays)
    try { set_error("C++ exception at the C boundary: %s", what ? what : "unknown type"); } catch (...) {}
    return LINNA_ERR_INTERNAL;
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return LINNA_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return LINNA_ERR_HIP;
}

static inline int ld4(int w) { return (w + 3) & ~3; }

// every element of a caller's layer array (the first entry's size is the array's stride: it is checked before walking on)
static int check_layers(const linna_layer_t* layers, int n, const char* who) {
    for (int i = 0; i < n; ++i) CHECK_STRUCT(layers + i, linna_layer_t, who);
    return LINNA_OK;
}
static int check_precision(int precision, const char* who) {
    if (precision == LINNA_PRECISION_FP32 || precision == LINNA_PRECISION_BF16) return LINNA_OK;
    set_error("%s: unknown precision %d (LINNA_PRECISION_FP32 0, LINNA_PRECISION_BF16 1)", who, precision);
    return LINNA_ERR_INVALID;
}
static bool capturing(void* stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(S(stream), &cap);
    return cap != hipStreamCaptureStatusNone;
}
// An environment switch reads `c` ('0' off, '1' on) NOW.  Every caller asks at the moment its object is created or first
// used; a process-wide cached value once made LINNA_DISABLE_FUSED dead for every object created after the first evaluation.
static bool env_is(const char* name, char c) {
    const char* e = getenv(name);
    return e && e[0] == c;
}
static GemmArgs gemm_zero() {
    GemmArgs a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (uint32_t)sizeof(GemmArgs);
    a.npairs = 1;
    a.alpha0 = 1.f;
    return a;
}
static void set_pair(GemmArgs& a, int i, const float* A, int lda, int alay, const float* B, int ldb, int blay, int K) {
    a.p[i].A = A; a.p[i].lda = lda; a.p[i].alay = alay;
    a.p[i].B = B; a.p[i].ldb = ldb; a.p[i].blay = blay; a.p[i].K = K;
}

}  // namespace linna

using namespace linna;

// Weight epoch: bumped by every entry that may change network parameters (linna_adamw_step, a
// graph replay, linna_weights_changed()); a log-probability object re-lays its fragment-order
// weight copy (net_stream.hip) when the epoch moved since the copy was made.
static std::atomic<unsigned long long> g_weights_epoch{1};

struct linna_ctx {
    int device;
    hipStream_t aux = nullptr;               // second stream: parameter-gradient GEMMs run beside the dX chain
    std::vector<hipEvent_t> events;          // fork/join markers (no timing)
    unsigned* counters = nullptr;            // zeroed, self-resetting arrival counters (fused loss)
    int loss_fused = -1;                     // -1 unknown, 0 off (env LINNA_LOSS_FUSED=0), 1 on
    void* comm = nullptr;                    // RCCL communicator state (comm.hip), set by linna_comm_init
};
void** linna_ctx_comm_slot(linna_ctx_t* ctx) { return &ctx->comm; }
int linna_ctx_device(const linna_ctx_t* ctx) { return ctx->device; }
struct linna_graph { hipGraph_t graph; hipGraphExec_t exec; };
// the auxiliary stream and the 2 * nl + 4 fork/join events a backward over nl ops uses
static int ctx_ensure_aux(linna_ctx* ctx, int nl) {
    if (!ctx->aux) TRY(check_hip(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking), "hipStreamCreate"));
    while ((int)ctx->events.size() < 2 * nl + 4) {
        hipEvent_t e;
        TRY(check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate"));
        ctx->events.push_back(e);
    }
    return LINNA_OK;
}

// The whole-network kernel (net_stream.hip) reads the weights from a copy in MFMA fragment order.  Its 16-row
// engine and its small-batch engines (8 / 4 rows per workgroup) read different orders, so there are two copies,
// each re-laid lazily when the weights moved (g_weights_epoch) since it was made.
struct StreamCopy {
    float* buf[2] = {nullptr, nullptr};      // [0]: 16-row engine, [1]: small-batch engines
    unsigned long long epoch[2] = {0, 0};    // epoch each copy was made at (0 = never)
    size_t floats = 0;
    bool ready() const { return buf[0] && buf[1]; }
    int alloc(size_t nf) {
        floats = nf;
        for (int k = 0; k < 2; ++k)
            if (hipMalloc(reinterpret_cast<void**>(&buf[k]), nf * sizeof(float)) != hipSuccess) { release(); return LINNA_ERR_HIP; }
        return LINNA_OK;
    }
    void release() {
        for (int k = 0; k < 2; ++k) { if (buf[k]) (void)hipFree(buf[k]); buf[k] = nullptr; epoch[k] = 0; }
    }
};

// What a training step of B rows trains through (net_train_mode): the weight streams an update has to write
enum TrainMode {
    TRAIN_NONE,          // no pair of whole-network streams (the step, where it runs, re-lays what it reads)
    TRAIN_FWD_DX,        // packed_loss (forward + loss) and packed_dx[0] (dX chain): two launches
    TRAIN_MERGED,        // packed_tb: forward + loss + dX chain in one launch (4-row engine)
    TRAIN_MERGED_BF16,   // packed_tbf: the same in bf16 (linna_net_set_train_precision)
};

struct linna_net {
    linna_ctx* ctx;

    StreamCopy packed;                       // fragment-order weight streams for the one-launch training forward
    int stream_fwd = -1;
    StreamCopy packed_loss;                  // ... for forward + chi^2-ratio loss in one launch (linna_net_forward_loss)
    NsDense loss_dn{nullptr, 0, nullptr, nullptr};   // the inverse covariance that stream ends in
    int stream_loss = -1;                    // -1 unknown, 0 no (not eligible), 1 yes
    StreamCopy packed_dx[2];                 // ... for the one-launch dX chain of the backward ([1]: down to the network input)
    StreamCopy packed_tb;                    // ... for forward + loss + dX chain in ONE launch (linna_net_train_step on the small-batch engines)
    int stream_tb = -1;                      // -1 unknown, 0 no (not eligible / LINNA_BWD_STREAM=0), 1 yes
    TrainMode as_mode = TRAIN_NONE;          // which streams as_args describes (TRAIN_NONE: none yet)
    int train_prec = LINNA_PRECISION_FP32;   // linna_net_set_train_precision: the form of the training step's network launch
    StreamCopy packed_tbf;                   // LINNA_PRECISION_BF16: the bf16 training stream (NS_TRAIN_STEP_BF16; [1] only, the 4-row engine)
    AsArgs as_args;                          // linna_net_adamw_step's descriptor table, valid for (as_params, as_n, as_k)
    const float* as_params = nullptr; size_t as_n = 0; int as_k = -1; int as_state = -1;   // as_state: -1 unknown, 0 unsupported, 1 ready
    int upd_state = -1; int upd_B = 0;       // linna_net_train_step_update: -1 unknown, 0 unsupported, 1 every parameter gradient of the step is in the grouped launch
    int stream_bwd[2] = {-1, -1};            // -1 unknown, 0 no (network out of reach / LINNA_BWD_STREAM=0), 1 yes
    std::vector<linna_layer_t> L;   // without the trailing INSKIP
    std::vector<linna_layer_t> Lfull;   // with it: what the serving programs of the whole-network kernel are built from
    int in_size, out_size;
    bool has_inskip;
    linna_layer_t inskip;
};
// the op list the programs of `kind` are planned from (ns_kind_full_layers), for the launchers
static NsNet net_layers(const linna_net* n, NsKind kind) {
    const std::vector<linna_layer_t>& L = ns_kind_full_layers(kind) ? n->Lfull : n->L;
    return NsNet{L.data(), (int)L.size(), n->in_size};
}

// The copy of `sc` that the engine of `rows` rows per workgroup reads, re-laid when the weights moved since it was made.
static int stream_copy_refresh(StreamCopy& sc, const linna_net* n, int rows, void* stream, const float** out, NsKind kind,
                               const NsDense* dn = nullptr) {
    const int k = rows < 16 ? 1 : 0;
    const unsigned long long epoch = g_weights_epoch.load();
    const bool cap = capturing(stream);
    if (cap || sc.epoch[k] != epoch) {
        // a captured launch carries its own re-layout, so that every replay sees the weights of that
        // moment; the copy is not valid for direct launches until they redo it (epoch 0)
        const NsNet net = net_layers(n, kind);
        TRY(launch_net_stream_pack(kind, net.layers, net.nl, net.in_size, sc.buf[k], rows, dn, S(stream)));
        sc.epoch[k] = cap ? 0 : epoch;
    }
    *out = sc.buf[k];
    return LINNA_OK;
}

// forward workspace: per op, the hidden h of a residual block, then the op's output (the last op's is the caller's)
static size_t fwd_floats(const linna_net* n, int B) {
    size_t f = 0;
    for (size_t i = 0; i < n->L.size(); ++i) {
        if (n->L[i].op == LINNA_OP_RESBLOCK) f += (size_t)B * ld4(n->L[i].C);
        if (i + 1 < n->L.size()) f += (size_t)B * ld4(n->L[i].N);
    }
    return f;
}
// Per op, where a training step's activations and their gradients live (NsOpBufs): the forward workspace `fwd_ws` in
// fwd_floats' order (the last op's output is `out`), and the backward workspace `bwd_ws` walked from the last op down --
// d/d(op input) for every op but the first (whose is `dX`, or none), d/dh behind it for a residual block.  No backward
// workspace: those entries stay unset.
static std::vector<NsOpBufs> net_bufs(const linna_net* n, int B, const float* X, int ldx, void* fwd_ws, float* out, int ldo,
                                      void* bwd_ws = nullptr, float* dX = nullptr, int lddx = 0) {
    const int nl = (int)n->L.size();
    float* w = static_cast<float*>(fwd_ws);
    size_t off = 0;
    std::vector<NsOpBufs> ops(nl, NsOpBufs{});
    for (int i = 0; i < nl; ++i) {
        const linna_layer_t& l = n->L[i];
        NsOpBufs& o = ops[i];
        const bool last = i == nl - 1;
        if (l.op == LINNA_OP_RESBLOCK) { o.t = w + off; off += (size_t)B * ld4(l.C); }
        o.ldt = ld4(l.C);
        if (last) { o.y = out; o.ldy = ldo; }
        else { o.y = w + off; o.ldy = ld4(l.N); off += (size_t)B * ld4(l.N); }
        o.x = i == 0 ? X : ops[i - 1].y; o.ldx = i == 0 ? ldx : ops[i - 1].ldy;
        // the input went through a ReLU iff the producing op is a resblock or a linear with relu
        o.gate = i > 0 && (n->L[i - 1].op == LINNA_OP_RESBLOCK || n->L[i - 1].relu) ? o.x : nullptr;
    }
    float* cur = static_cast<float*>(bwd_ws);
    for (int i = nl - 1; i >= 0 && cur; --i) {
        const linna_layer_t& l = n->L[i];
        ops[i].dprev = i == 0 ? dX : cur; ops[i].ldp = i == 0 ? lddx : ld4(l.K);
        if (i > 0) cur += (size_t)B * ld4(l.K);
        if (l.op == LINNA_OP_RESBLOCK) { ops[i].dt = cur; ops[i].lddt = ld4(l.C); cur += (size_t)B * ld4(l.C); }
    }
    return ops;
}

extern "C" {

// ------------------------------------------------------------------ runtime
int linna_abi_version(void) { return LINNA_ABI_VERSION; }
const char* linna_last_error(void) { return g_err.c_str(); }
// diagnostic: raise inside a guarded entry (tests/test_abi.py checks that the barrier turns it into a code and a text)
int linna_debug_raise(int kind) try {
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) { std::vector<int> v; v.reserve(v.max_size() + 1); }      // std::length_error, as a planner's vector would
    if (kind == 3) throw 42;                                                  // not derived from std::exception
    if (kind == 4) { std::string s; (void)s.at(7); }                          // std::out_of_range
    return LINNA_OK;
} LINNA_CATCH_INT

int linna_ctx_create(int device, linna_ctx_t** out) try {
    if (!out) { set_error("ctx_create: null out"); return LINNA_ERR_INVALID; }
    int n = 0;
    TRY(check_hip(hipGetDeviceCount(&n), "hipGetDeviceCount"));
    if (device < 0 || device >= n) { set_error("ctx_create: device %d of %d", device, n); return LINNA_ERR_INVALID; }
    hipDeviceProp_t prop;
    TRY(check_hip(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties"));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        set_error("ctx_create: device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return LINNA_ERR_UNSUPPORTED;
    }
    linna_ctx* c = new (std::nothrow) linna_ctx();
    if (!c) return LINNA_ERR_INVALID;
    c->device = device;
    // the context's device-side state is allocated HERE, so that no launch ever allocates: the arrival counters of the
    // one-launch loss
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = check_hip(hipSetDevice(device), "hipSetDevice");
    if (rc == LINNA_OK) rc = check_hip(hipMalloc(reinterpret_cast<void**>(&c->counters), 64), "hipMalloc(counters)");
    if (rc == LINNA_OK) rc = check_hip(hipMemset(c->counters, 0, 64), "hipMemset(counters)");
    (void)hipSetDevice(prev);
    if (rc != LINNA_OK) { (void)linna_ctx_destroy(c); return rc; }
    *out = c;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_ctx_destroy(linna_ctx_t* ctx) try {
    if (ctx) {
        (void)linna_comm_destroy(ctx);
        for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
        if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
        if (ctx->counters) (void)hipFree(ctx->counters);
    }
    delete ctx;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_stream_sync(void* stream) try { return check_hip(hipStreamSynchronize(S(stream)), "hipStreamSynchronize"); } LINNA_CATCH_INT

int linna_graph_begin(void* stream) try {
    return check_hip(hipStreamBeginCapture(S(stream), hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
} LINNA_CATCH_INT
int linna_graph_end(void* stream, linna_graph_t** out) try {
    hipGraph_t g = nullptr;
    TRY(check_hip(hipStreamEndCapture(S(stream), &g), "hipStreamEndCapture"));
    hipGraphExec_t e = nullptr;
    int rc = check_hip(hipGraphInstantiate(&e, g, nullptr, nullptr, 0), "hipGraphInstantiate");
    if (rc != LINNA_OK) { (void)hipGraphDestroy(g); return rc; }
    *out = new linna_graph{g, e};
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_graph_launch(linna_graph_t* g, void* stream) try {
    if (!g) { set_error("graph_launch: null graph"); return LINNA_ERR_INVALID; }
    g_weights_epoch.fetch_add(1);            // the graph may hold an AdamW step
    return check_hip(hipGraphLaunch(g->exec, S(stream)), "hipGraphLaunch");
} LINNA_CATCH_INT
int linna_graph_destroy(linna_graph_t* g) try {
    if (!g) return LINNA_OK;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_event_create(void** ev) try {
    hipEvent_t e;
    TRY(check_hip(hipEventCreate(&e), "hipEventCreate"));
    *ev = e;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_event_record(void* ev, void* stream) try { return check_hip(hipEventRecord((hipEvent_t)ev, S(stream)), "hipEventRecord"); } LINNA_CATCH_INT
int linna_event_elapsed_ms(void* a, void* b, float* ms) try {
    TRY(check_hip(hipEventSynchronize((hipEvent_t)b), "hipEventSynchronize"));
    return check_hip(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b), "hipEventElapsedTime");
} LINNA_CATCH_INT
int linna_event_destroy(void* ev) try { return check_hip(hipEventDestroy((hipEvent_t)ev), "hipEventDestroy"); } LINNA_CATCH_INT

// ------------------------------------------------------------------ GEMM
int linna_gemm_f32(linna_ctx_t*, const linna_gemm_t* d, void* stream) try {
    if (!d) { set_error("gemm: null descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_gemm_t, "gemm");
    return gemm_launch(*d, S(stream));
} LINNA_CATCH_INT
int linna_gemm_dot_slots(int M, int N) try { return gemm_slots(M, N); } LINNA_CATCH_INT

// ------------------------------------------------------------------ layers
int linna_linear_fwd(linna_ctx_t*, const float* X, int ldx, const float* W, int ldw, const float* b, float* Y, int ldy,
                     int B, int K, int N, int relu, float alpha, const float* R, int ldr, void* stream) try {
    GemmArgs a = gemm_zero();
    set_pair(a, 0, X, ldx, LAY_K, W, ldw, LAY_K, K);
    a.M = B; a.N = N; a.C = Y; a.ldc = ldy; a.bias0 = b; a.alpha0 = alpha; a.R = R; a.ldr = ldr; a.relu = relu;
    return gemm_launch(a, S(stream));
} LINNA_CATCH_INT

int linna_resblock_fwd(linna_ctx_t*, const float* X, int ldx, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* Ws, float* T, int ldt, float* Y, int ldy, int B, int K, int C,
                       int N, void* stream) try {
    if (!Ws && K != N) { set_error("resblock: identity skip needs K == N"); return LINNA_ERR_INVALID; }
    TRY(linna_linear_fwd(nullptr, X, ldx, W1, ld4(K), b1, T, ldt, B, K, C, 1, 1.f, nullptr, 0, stream));
    GemmArgs a = gemm_zero();
    set_pair(a, 0, T, ldt, LAY_K, W2, ld4(C), LAY_K, C);
    a.M = B; a.N = N; a.C = Y; a.ldc = ldy; a.bias0 = b2; a.alpha0 = 0.1f; a.relu = 1;
    if (Ws) { a.npairs = 2; set_pair(a, 1, X, ldx, LAY_K, Ws, ld4(K), LAY_K, K); }
    else { a.R = X; a.ldr = ldx; }
    return gemm_launch(a, S(stream));
} LINNA_CATCH_INT

int linna_linear_bwd(linna_ctx_t*, const float* dY, int lddy, const float* X, int ldx, const float* W, int ldw,
                     float* dX, int lddx, const float* Xmask, int ldxm, float* dW, int lddw, float* db, int B, int K,
                     int N, float scale, void* stream) try {
    if (dW) {   // dW[n][k] = scale * sum_b dY[b][n] X[b][k]
        GemmArgs a = gemm_zero();
        set_pair(a, 0, dY, lddy, LAY_MN, X, ldx, LAY_MN, B);
        a.M = N; a.N = K; a.C = dW; a.ldc = lddw; a.alpha0 = scale;
        TRY(gemm_launch(a, S(stream)));
    }
    if (db) TRY(launch_colsum(dY, lddy, B, N, scale, db, S(stream)));
    if (dX) {   // dX[b][k] = scale * sum_n dY[b][n] W[n][k]
        GemmArgs a = gemm_zero();
        set_pair(a, 0, dY, lddy, LAY_K, W, ldw, LAY_MN, N);
        a.M = B; a.N = K; a.C = dX; a.ldc = lddx; a.alpha0 = scale; a.mask = Xmask; a.ldmask = ldxm;
        TRY(gemm_launch(a, S(stream)));
    }
    return LINNA_OK;
} LINNA_CATCH_INT

// ------------------------------------------------------------------ network
int linna_net_create(linna_ctx_t* ctx, const linna_layer_t* layers, int nlayers, int in_size, linna_net_t** out) try {
    if (!layers || nlayers < 1 || !out) { set_error("net_create: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "net_create"));
    linna_net* n = new linna_net();
    n->ctx = ctx; n->in_size = in_size; n->has_inskip = false;
    int width = in_size;
    for (int i = 0; i < nlayers; ++i) {
        const linna_layer_t& l = layers[i];
        if (l.op == LINNA_OP_INSKIP) {
            if (i != nlayers - 1 || l.K != in_size || l.N != width) {
                set_error("net_create: INSKIP must be the last op, K = in_size, N = network width");
                delete n; return LINNA_ERR_INVALID;
            }
            n->has_inskip = true; n->inskip = l;
            continue;
        }
        if (l.K != width) { set_error("net_create: op %d expects K=%d, got %d", i, width, l.K); delete n; return LINNA_ERR_INVALID; }
        if (l.op == LINNA_OP_RESBLOCK) {
            if (!l.Ws && l.K != l.N) { set_error("net_create: op %d identity skip with K != N", i); delete n; return LINNA_ERR_INVALID; }
        } else if (l.op != LINNA_OP_LINEAR) { set_error("net_create: unknown op %d", l.op); delete n; return LINNA_ERR_INVALID; }
        width = l.N;
        n->L.push_back(l);
    }
    const linna_layer_t& last = n->L.back();
    if (last.op != LINNA_OP_LINEAR || last.relu) {
        set_error("net_create: the last op must be a LINEAR without ReLU"); delete n; return LINNA_ERR_INVALID;
    }
    if (n->has_inskip && n->L[0].op != LINNA_OP_LINEAR) {
        set_error("net_create: INSKIP needs a LINEAR first op"); delete n; return LINNA_ERR_INVALID;
    }
    n->out_size = width;
    n->Lfull = n->L;
    if (n->has_inskip) n->Lfull.push_back(n->inskip);
    *out = n;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_net_destroy(linna_net_t* net) try {
    if (net) {
        net->packed.release(); net->packed_dx[0].release(); net->packed_dx[1].release(); net->packed_loss.release();
        net->packed_tb.release(); net->packed_tbf.release();
    }
    delete net;
    return LINNA_OK;
} LINNA_CATCH_INT

// Device-side weight copies of the one-launch paths (net_stream.hip): decided once per network, allocated by
// linna_net_prepare -- or on first use, when the caller did not prepare and the stream is not capturing.
static void net_ensure_fwd(linna_net* n, bool may_alloc) {
    const int nl = (int)n->L.size();
    if (n->stream_fwd < 0) {
        n->stream_fwd = !n->has_inskip && !env_is("LINNA_FWD_STREAM", '0') && net_stream_plan(NS_STORE, n->L.data(), nl, n->in_size).ok ? 1 : 0;
    }
    if (n->stream_fwd == 1 && !n->packed.ready() && may_alloc) {
        if (n->packed.alloc(net_stream_plan(NS_STORE, n->L.data(), nl, n->in_size).packed_floats) != LINNA_OK) n->stream_fwd = 0;
    }
}
static void net_ensure_dx(linna_net* n, int wi, bool may_alloc) {
    const int nl = (int)n->L.size();
    const NsKind kind = wi ? NS_DX_INPUT : NS_DX;
    if (n->stream_bwd[wi] < 0) {
        n->stream_bwd[wi] = !n->has_inskip && (nl >= 2 || wi) && !env_is("LINNA_BWD_STREAM", '0') &&
                            net_stream_plan(kind, n->L.data(), nl, n->in_size).ok ? 1 : 0;
    }
    StreamCopy& sc = n->packed_dx[wi];
    if (n->stream_bwd[wi] == 1 && !sc.ready() && may_alloc) {
        if (sc.alloc(net_stream_plan(kind, n->L.data(), nl, n->in_size).packed_floats) != LINNA_OK) n->stream_bwd[wi] = 0;
    }
}
int linna_net_prepare(linna_net_t* n, int backward, int input_grad) try {
    if (!n) { set_error("net_prepare: null network"); return LINNA_ERR_INVALID; }
    net_ensure_fwd(n, true);
    if (backward) net_ensure_dx(n, input_grad ? 1 : 0, true);
    if (n->ctx && backward) TRY(ctx_ensure_aux(n->ctx, (int)n->L.size()));      // for the same reason
    return LINNA_OK;
} LINNA_CATCH_INT

size_t linna_net_fwd_ws_bytes(const linna_net_t* n, int B) try { return (fwd_floats(n, B) + 16) * sizeof(float); } LINNA_CATCH_SIZE
// backward scratch: one buffer per op for the gradient wrt that op's input (no reuse: the
// parameter-gradient GEMMs of an op may still be reading it on the auxiliary stream while the dX
// chain moves on) + one dT buffer per residual block
static size_t bwd_floats(const linna_net* n, int B) {
    size_t f = 0;
    for (size_t i = 0; i < n->L.size(); ++i) {
        f += (size_t)B * ld4(n->L[i].K);
        if (n->L[i].op == LINNA_OP_RESBLOCK) f += (size_t)B * ld4(n->L[i].C);
    }
    return f;
}
size_t linna_net_bwd_ws_bytes(const linna_net_t* n, int B) try { return (bwd_floats(n, B) + 16) * sizeof(float); } LINNA_CATCH_SIZE

int linna_net_forward(linna_net_t* n, const float* X, int ldx, int B, void* ws, float* OUT, int ldo,
                      const linna_colmap_t* om, void* stream) try {
    if (!n || !X || !OUT || B < 1) { set_error("net_forward: bad arguments"); return LINNA_ERR_INVALID; }
    float* w = static_cast<float*>(ws);
    const int nl = (int)n->L.size();
    if (nl > 1 && !w) { set_error("net_forward: workspace required"); return LINNA_ERR_INVALID; }
    const std::vector<NsOpBufs> ops = net_bufs(n, B, X, ldx, w, OUT, ldo);
    if ((!om || !om->cexp) && !n->has_inskip) {
        // ONE launch (net_stream.hip, STORE): at batch 500 the ten layer GEMMs are 10-30 us of latency each.  The
        // fragment-order weight copy is re-laid whenever the weights moved (every optimiser step: ~10 us).
        net_ensure_fwd(n, !capturing(stream));
        if (n->stream_fwd == 1 && n->packed.ready()) {
            const int rows = net_stream_rows(B);
            const float* packed = nullptr;
            TRY(stream_copy_refresh(n->packed, n, rows, stream, &packed, NS_STORE));
            return launch_net_stream_store(net_layers(n, NS_STORE), packed, X, ldx, B, ops.data(), om ? om->cscale : nullptr,
                                           om ? om->cshift : nullptr, rows, S(stream));
        }
    }
    const float* hin = X; int ldh = ldx;
    for (int i = 0; i < nl; ++i) {
        const linna_layer_t& l = n->L[i];
        const bool last = (i == nl - 1);
        float* Y = ops[i].y;
        const int ldy = ops[i].ldy;
        if (l.op == LINNA_OP_LINEAR) {
            GemmArgs a = gemm_zero();
            a.M = B; a.N = l.N; a.C = Y; a.ldc = ldy; a.relu = l.relu;
            if (last && n->has_inskip) {
                // out = (hin W^T + b) + alpha * (X0 Wl^T + bl): pair 0 carries the scaled input skip
                const linna_layer_t& s = n->inskip;
                a.npairs = 2;
                set_pair(a, 0, X, ldx, LAY_K, s.W, ld4(s.K), LAY_K, s.K);
                a.bias0 = s.b; a.alpha0 = s.alpha;
                set_pair(a, 1, hin, ldh, LAY_K, l.W, ld4(l.K), LAY_K, l.K);
                a.bias1 = l.b;
            } else {
                set_pair(a, 0, hin, ldh, LAY_K, l.W, ld4(l.K), LAY_K, l.K);
                a.bias0 = l.b;
            }
            if (last && om) {
                a.cscale = om->cscale; a.cshift = om->cshift; a.cexp = om->cexp; a.cpost = om->cpost; a.cshift2 = om->cshift2;
            }
            TRY(gemm_launch(a, S(stream)));
        } else {
            TRY(linna_resblock_fwd(nullptr, hin, ldh, l.W1, l.b1, l.W2, l.b2, l.Ws, ops[i].t, ops[i].ldt, Y, ldy, B, l.K, l.C, l.N, stream));
        }
        hin = Y; ldh = ldy;
    }
    return LINNA_OK;
} LINNA_CATCH_INT

static bool net_loss_stale(const linna_net* n, const NsDense& dn) { return n->stream_loss < 0 || n->loss_dn.S != dn.S || n->loss_dn.lds != dn.lds; }
static void net_ensure_loss(linna_net* n, const NsDense& dn) {
    const int nl = (int)n->L.size();
    const NsPlan loss = net_stream_plan(NS_TRAIN_FWD, n->L.data(), nl, n->in_size, &dn);
    const bool ok = !n->has_inskip && loss.ok;
    n->packed_loss.release();
    n->stream_loss = 0; n->loss_dn = dn;
    if (ok && n->packed_loss.alloc(loss.packed_floats) == LINNA_OK) n->stream_loss = 1;
    // the same loss behind the one-launch training step (forward + loss + dX chain in one weight stream)
    const NsPlan merged = ok && n->stream_loss == 1 && !env_is("LINNA_BWD_STREAM", '0') && nl >= 2 ? net_stream_plan(NS_TRAIN_STEP, n->L.data(), nl, n->in_size, &dn)
                                                                                            : NsPlan{false, 0, false, nullptr};
    n->packed_tb.release();
    n->packed_tbf.epoch[0] = n->packed_tbf.epoch[1] = 0;     // (the bf16 stream holds the loss's inverse covariance too)
    n->stream_tb = 0; n->as_mode = TRAIN_NONE; n->as_state = -1;
    if (merged.ok && n->packed_tb.alloc(merged.packed_floats) == LINNA_OK) n->stream_tb = 1;
}
// The streams must end in the loss `d`: (re)built when it is not the one they were built for -- outside a stream capture only
static int net_loss_current(linna_net* n, const linna_loss_desc_t* d, void* stream, const char* who) {
    const NsDense dn{d->Cinv, d->ldc, nullptr, nullptr};
    if (!net_loss_stale(n, dn)) return LINNA_OK;
    if (capturing(stream)) {
        set_error("%s: first use inside a stream capture (call linna_net_prepare_loss before)", who); return LINNA_ERR_UNSUPPORTED;
    }
    net_ensure_loss(n, dn);
    return LINNA_OK;
}
// A bf16 net (linna_net_set_train_precision): the training entries run the bf16 step or return LINNA_ERR_UNSUPPORTED with the
// reason -- never the fp32 one
static bool net_bf16(const linna_net* n) { return n->train_prec == LINNA_PRECISION_BF16; }
// THE decision of what a step of B rows trains through, for every entry that touches the training streams (train_launches,
// train_step, train_step_update, adamw_step).  The merged forms serve the 4-row engine only (batches of up to 1024 rows).
static TrainMode net_train_mode(const linna_net* n, int B) {
    const bool four = net_stream_rows(B) == 4;
    if (net_bf16(n)) return n->packed_tbf.ready() && four && n->loss_dn.S ? TRAIN_MERGED_BF16 : TRAIN_NONE;
    if (n->stream_loss != 1) return TRAIN_NONE;
    if (n->stream_tb == 1 && n->packed_tb.ready() && four) return TRAIN_MERGED;
    return n->stream_bwd[0] == 1 ? TRAIN_FWD_DX : TRAIN_NONE;
}
// why a bf16 net has no mode for this batch, in the entry's name (an fp32 net, or a bf16 one with its mode: fine)
static int net_bf16_mode_check(const linna_net* n, int B, const char* who) {
    if (!net_bf16(n) || net_train_mode(n, B) == TRAIN_MERGED_BF16) return LINNA_OK;
    if (!n->packed_tbf.ready()) { set_error("%s: bf16 training stream not allocated", who); return LINNA_ERR_UNSUPPORTED; }
    if (net_stream_rows(B) != 4) {
        set_error("%s: the bf16 training step runs on the 4-row engine only; a batch of %d rows needs the %d-row engine", who, B, net_stream_rows(B));
        return LINNA_ERR_UNSUPPORTED;
    }
    set_error("%s: bf16 training stream: no loss seen yet (linna_net_prepare_loss)", who);
    return LINNA_ERR_UNSUPPORTED;
}
// The streams of a mode: `fwd` of program `kind` (forward + loss, with the dX chain when merged), `dx` the dX chain's own or null
struct TrainStreams { StreamCopy* fwd; NsKind kind; StreamCopy* dx; };
static TrainStreams net_train_streams(linna_net* n, TrainMode mode) {
    if (mode == TRAIN_MERGED_BF16) return TrainStreams{&n->packed_tbf, NS_TRAIN_STEP_BF16, nullptr};
    if (mode == TRAIN_MERGED) return TrainStreams{&n->packed_tb, NS_TRAIN_STEP, nullptr};
    return TrainStreams{&n->packed_loss, NS_TRAIN_FWD, &n->packed_dx[0]};
}
// An update has just written the mode's streams for the engine of B rows: they hold the new weights.  (A captured update
// stamps nothing: every replay's launches carry their own re-layout.)
static void net_stamp_updated(linna_net* n, TrainMode mode, int B, void* stream) {
    const unsigned long long epoch = g_weights_epoch.fetch_add(1) + 1;
    if (capturing(stream)) return;
    const int k = net_stream_rows(B) < 16 ? 1 : 0;
    const TrainStreams ts = net_train_streams(n, mode);
    ts.fwd->epoch[k] = epoch;
    if (ts.dx) ts.dx->epoch[k] = epoch;
}
int linna_loss_targets(linna_ctx_t*, const linna_loss_desc_t* d, const float* Y, int ldy, int nrows, float* YN, int ldyn, void* stream) try {
    if (!d || !Y || !YN || nrows < 1) { set_error("loss_targets: bad arguments"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "loss_targets");
    if (ldyn < d->nout) { set_error("loss_targets: ldyn %d < nout %d", ldyn, d->nout); return LINNA_ERR_INVALID; }
    return launch_loss_targets(Y, ldy, nrows, *d, YN, ldyn, S(stream));
} LINNA_CATCH_INT
int linna_net_prepare_loss(linna_net_t* n, const linna_loss_desc_t* d) try {
    if (!n || !d) { set_error("net_prepare_loss: null argument"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "net_prepare_loss");
    const NsDense dn{d->Cinv, d->ldc, nullptr, nullptr};
    if (net_loss_stale(n, dn)) net_ensure_loss(n, dn);
    return LINNA_OK;
} LINNA_CATCH_INT

// The arguments the three training-step entries share, filled once per call: the batch, the loss and where its results go,
// the workspaces (bwd_ws: null for linna_net_forward_loss), the network output PRED, the batch mean's slot and the AdamW
// state whose step constants the step advances (hyper / step_dev null: none).
struct TrainStep {
    NsBatch b; NsTrainLoss loss;
    void* fwd_ws; void* bwd_ws; float* PRED; int ldp;
    float* loss_mean; float* hyper; int* step_dev; float b1, b2;
};
// the step's two single-thread jobs (NsPost): the batch mean of the loss rows, AdamW's step counter and bias corrections
static NsPost train_riders(const TrainStep& t) {
    const bool prep = t.hyper && t.step_dev;
    return NsPost{t.loss.loss_rows, t.b.B, t.loss.inv_batch, t.loss_mean, prep ? t.step_dev : nullptr, prep ? t.hyper : nullptr, t.b1, t.b2};
}
// ... as a launch of their own, where no whole-network launch carries them (both jobs: one launch)
static int launch_riders(const NsPost& p, hipStream_t st) {
    if (p.out && p.step) return launch_sum_scale_prepare(p.rows, p.n, p.scale, p.out, p.step, p.hyper, p.b1, p.b2, st);
    if (p.out) return launch_sum_scale(p.rows, p.n, p.scale, p.out, st);
    if (p.step) return launch_adamw_prepare(p.hyper, p.step, p.b1, p.b2, st);
    return LINNA_OK;
}

struct NetUpdate { float* params; float* m; float* v; float* hyper; float b1, b2, eps; bool bf; };   // bf: the bf16 training stream's writer
// What rides with a backward:
// `post`: the loss mean / AdamW step constants of this step (linna_net_train_step): they ride in the one-launch dX chain
// as an extra workgroup, or run as the launch of their own they otherwise are, in front of the GEMM chain
// `upd`: the optimiser rides in the grouped parameter-gradient launch (linna_net_train_step_update; the caller has checked
// upd_state: every parameter gradient of the step goes into that launch)
// `dx_done`: the dX chain already ran (inside the one-launch training step): only the parameter gradients are left;
// `gpost`: the batch mean of the loss rows rides in the grouped parameter-gradient launch as one extra workgroup
struct BwdRiders { const NsPost* post = nullptr; const NetUpdate* upd = nullptr; bool dx_done = false; const GemmPost* gpost = nullptr; };
static int net_backward_impl(linna_net_t* n, const float* X, int ldx, int B, void* fwd_ws, void* bwd_ws, const float* dOUT,
                             int lddo, float* dX, int lddx, int pg, void* stream, const BwdRiders& riders) {
    const NsPost* const post = riders.post;
    const NetUpdate* const upd = riders.upd;
    const GemmPost* gpost = riders.gpost;     // (handed to the first launch that can carry it)
    if (!n || !X || !dOUT || !bwd_ws || B < 1) { set_error("net_backward: bad arguments"); return LINNA_ERR_INVALID; }
    const std::vector<NsOpBufs> ops = net_bufs(n, B, X, ldx, fwd_ws, nullptr, 0, bwd_ws, dX, lddx);
    const int nl = (int)n->L.size();
    hipStream_t st = S(stream);

    // ---- with a context: an auxiliary stream for the parameter gradients (off the dX critical path), and the dW GEMMs
    // (1-128 tiles each, 251 together for ChtoModelv2(33,33)) collected and launched as ONE grid after the dX chain --
    // 13 launches of ~18 us each on the auxiliary stream were the critical path of the step.  What does not fit that grid
    // goes to the auxiliary stream as it becomes possible.
    linna_ctx* ctx = n->ctx;
    const bool overlap = pg && ctx;
    if (overlap) TRY(ctx_ensure_aux(ctx, nl));
    int next_event = 0;
    void* aux = overlap ? (void*)ctx->aux : stream;
    GemmGroupArgs grp;                  // the grouped parameter-gradient launch: descriptors by value, filled as we go
    grp.nprob = 0;
    GemmGroupArgsS grpu;                // ... and its form with the optimiser in the epilogue
    GemmUpdate gu;
    grpu.nprob = 0;
    long long pdiff = 0;
    if (upd) {
        ::memset(static_cast<void*>(&gu), 0, sizeof(gu));
        const linna_layer_t& l0 = n->L[0];
        const float* w0 = l0.op == LINNA_OP_RESBLOCK ? l0.W1 : l0.W;
        const float* g0 = l0.op == LINNA_OP_RESBLOCK ? l0.gW1 : l0.gW;
        pdiff = w0 - g0;
        gu.pdiff = pdiff; gu.mdiff = (upd->m - upd->params) + pdiff; gu.vdiff = (upd->v - upd->params) + pdiff;
        gu.hyper = upd->hyper; gu.beta1 = upd->b1; gu.beta2 = upd->b2; gu.eps = upd->eps; gu.small = n->as_args.small;
    }
    auto as_range_of = [&](const float* param, int kind) -> const AsRange* {     // the flat-buffer tensor that starts at `param`
        const long long off = param - upd->params;
        for (int i = 0; i < n->as_args.nr; ++i)
            if (n->as_args.r[i].kind == kind && (long long)n->as_args.r[i].off4 * 4 == off) return &n->as_args.r[i];
        return nullptr;
    };
    int grp_blocks = 0;
    bool aux_used = false;
    auto fork = [&]() -> int {       // work enqueued on aux after this sees everything enqueued on st so far
        if (!overlap) return LINNA_OK;
        aux_used = true;
        hipEvent_t e = ctx->events[next_event++];
        TRY(check_hip(hipEventRecord(e, st), "hipEventRecord"));
        return check_hip(hipStreamWaitEvent(ctx->aux, e, 0), "hipStreamWaitEvent");
    };
    auto param_grads = [&](const float* dY, int lddy, const float* Xin, int ldxin, float* dW, int lddw, float* db, int K,
                           int N, float scale) -> int {
        GemmArgs a = gemm_zero();    // dW[n][k] = scale * sum_b dY[b][n] X[b][k]
        set_pair(a, 0, dY, lddy, LAY_MN, Xin, ldxin, LAY_MN, B);
        a.M = N; a.N = K; a.C = dW; a.ldc = lddw; a.alpha0 = scale;
        if (upd) {
            if (!(overlap && grpu.nprob < GEMM_UPD_MAX && gemm_group_ok(a))) { set_error("net_backward: update outside the grouped launch"); return LINNA_ERR_INVALID; }
            const AsRange* rw = as_range_of(dW + pdiff, 0);
            const AsRange* rb = db ? as_range_of(db + pdiff, 1) : nullptr;
            if (!rw || (db && !rb)) { set_error("net_backward: update of a tensor outside the flat parameter buffer"); return LINNA_ERR_INVALID; }
            const int i = grpu.nprob++;
            grpu.p[i] = GemmGroupProb{dY, Xin, dW, db, lddy, ldxin, lddw, B, N, K, scale, grp_blocks};
            gu.pl[i][0] = n->as_args.w[rw->idx].pl[0]; gu.pl[i][1] = n->as_args.w[rw->idx].pl[1];
            if (rb) gu.bias[i] = n->as_args.b[rb->idx];
            grp_blocks += gemm_group_blocks(a);
            return LINNA_OK;
        }
        if (overlap && grp.nprob < GEMM_GROUP_MAX && gemm_group_ok(a)) {
            // one tile grid for every dW of the step; the bias gradient (column sums of dY) rides in the same tiles
            grp.p[grp.nprob++] = GemmGroupProb{dY, Xin, dW, db, lddy, ldxin, lddw, B, N, K, scale, grp_blocks};
            grp_blocks += gemm_group_blocks(a);
            return LINNA_OK;
        }
        TRY(fork()); TRY(gemm_launch(a, S(aux)));
        if (db) { TRY(fork()); TRY(launch_colsum(dY, lddy, B, N, scale, db, S(aux))); }
        return LINNA_OK;
    };

    if (n->has_inskip && pg) {
        const linna_layer_t& s = n->inskip;
        TRY(param_grads(dOUT, lddo, X, ldx, s.gW, ld4(s.K), s.gb, s.K, s.N, s.alpha));
    }
    // The dX chain -- one GEMM per op, each waiting for the one before (140 us of 300 at batch 500) -- as ONE launch of
    // the whole-network kernel over the transposed weights (net_stream.hip, STORE == 2), when the network has such a
    // program.  The loop below then only collects the parameter gradients.
    bool fused_dx = riders.dx_done;
    const int wi = dX ? 1 : 0;
    if (!riders.dx_done && !n->has_inskip && (nl >= 2 || dX)) {
        net_ensure_dx(n, wi, !capturing(stream));
        StreamCopy& sc = n->packed_dx[wi];
        if (n->stream_bwd[wi] == 1 && sc.ready()) {
            const int rows = net_stream_rows(B);
            const float* packed = nullptr;
            TRY(stream_copy_refresh(sc, n, rows, stream, &packed, wi ? NS_DX_INPUT : NS_DX));
            TRY(launch_net_stream_dx(net_layers(n, NS_DX), packed, dOUT, lddo, B, ops.data(), wi, rows, st, post));
            fused_dx = true;
        }
    }
    if (post && !fused_dx) TRY(launch_riders(*post, st));
    const float* dcur = dOUT; int ldd = lddo;
    for (int i = nl - 1; i >= 0; --i) {
        const linna_layer_t& l = n->L[i];
        const float* hin = ops[i].x;
        const int ldh = ops[i].ldx;
        const bool need_dx = (i > 0) || (dX != nullptr);
        float* dprev = ops[i].dprev;
        const int ldp = ops[i].ldp;
        const float* mask = ops[i].gate;
        if (l.op == LINNA_OP_LINEAR) {
            if (pg) {                // dW, db need only dcur (already produced on st) and hin
                TRY(param_grads(dcur, ldd, hin, ldh, l.gW, ld4(l.K), l.gb, l.K, l.N, 1.f));
            }
            if (need_dx && !fused_dx) {
                GemmArgs a = gemm_zero();
                a.M = B; a.N = l.K; a.C = dprev; a.ldc = ldp; a.mask = mask; a.ldmask = ldh;
                if (i == 0 && n->has_inskip) {
                    const linna_layer_t& s = n->inskip;
                    a.npairs = 2;
                    set_pair(a, 0, dOUT, lddo, LAY_K, s.W, ld4(s.K), LAY_MN, s.N);
                    a.alpha0 = s.alpha;
                    set_pair(a, 1, dcur, ldd, LAY_K, l.W, ld4(l.K), LAY_MN, l.N);
                } else {
                    set_pair(a, 0, dcur, ldd, LAY_K, l.W, ld4(l.K), LAY_MN, l.N);
                }
                TRY(gemm_launch(a, st));
            }
        } else {
            const float* T = ops[i].t;
            const int ldt = ops[i].ldt;
            float* dT = ops[i].dt;
            if (!fused_dx) {   // dT = 0.1 * (dcur W2) * (T > 0)
                GemmArgs a = gemm_zero();
                set_pair(a, 0, dcur, ldd, LAY_K, l.W2, ld4(l.C), LAY_MN, l.N);
                a.M = B; a.N = l.C; a.C = dT; a.ldc = ldt; a.alpha0 = 0.1f; a.mask = T; a.ldmask = ldt;
                TRY(gemm_launch(a, st));
            }
            if (pg) {
                TRY(param_grads(dcur, ldd, T, ldt, l.gW2, ld4(l.C), l.gb2, l.C, l.N, 0.1f));   // (after dT)
                TRY(param_grads(dT, ldt, hin, ldh, l.gW1, ld4(l.K), l.gb1, l.K, l.C, 1.f));
                if (l.Ws) TRY(param_grads(dcur, ldd, hin, ldh, l.gWs, ld4(l.K), nullptr, l.K, l.N, 1.f));
            }
            if (need_dx && !fused_dx) {   // dprev = (dT W1 + dcur Ws [+ dcur]) * (hin > 0)
                GemmArgs a = gemm_zero();
                set_pair(a, 0, dT, ldt, LAY_K, l.W1, ld4(l.K), LAY_MN, l.C);
                a.M = B; a.N = l.K; a.C = dprev; a.ldc = ldp; a.mask = mask; a.ldmask = ldh;
                if (l.Ws) { a.npairs = 2; set_pair(a, 1, dcur, ldd, LAY_K, l.Ws, ld4(l.K), LAY_MN, l.N); }
                else { a.R = dcur; a.ldr = ldd; }
                TRY(gemm_launch(a, st));
            }
        }
        dcur = dprev; ldd = ldp;
    }
    if (grp.nprob) { TRY(gemm_launch_group(grp, grp_blocks, st, gpost)); gpost = nullptr; }     // every dY is on `st` by now: one grid over all the dW tiles
    if (grpu.nprob) { TRY(gemm_launch_group_update(grpu, gu, grp_blocks, st, gpost, upd && upd->bf)); gpost = nullptr; }
    if (gpost && gpost->n > 0) TRY(launch_sum_scale(gpost->rows, gpost->n, gpost->scale, gpost->out, st));   // (no grouped launch to ride in)
    if (overlap && aux_used) {       // join: the caller's stream continues only after every gradient is written
        hipEvent_t e = ctx->events[next_event++];
        TRY(check_hip(hipEventRecord(e, ctx->aux), "hipEventRecord"));
        TRY(check_hip(hipStreamWaitEvent(st, e, 0), "hipStreamWaitEvent"));
    }
    return LINNA_OK;
}
// the backward of a training step on the rows its forward gathered: every parameter gradient, no input gradient
static int net_train_backward(linna_net_t* n, const TrainStep& t, void* stream, const BwdRiders& riders) {
    return net_backward_impl(n, t.b.XB, t.b.ldxb, t.b.B, t.fwd_ws, t.bwd_ws, t.loss.dP, t.loss.lddp, nullptr, 0, 1, stream, riders);
}

// linna_net_forward_loss (linna_hip.h): the batch rows are gathered from the resident set and X-transformed in the kernel's
// prologue, every activation the backward needs is stored, the network's normalised-space inverse covariance is the
// program's last segment and the finish writes the per-row loss and d loss / d pred (net_stream.hip, STORE == 3).  The
// riders are a second, tiny launch (fixed summation order) -- or, `defer_post`, left to the backward's dX launch.
static int net_forward_loss_impl(linna_net_t* n, const linna_loss_desc_t* d, const TrainStep& t, void* stream, bool defer_post) {
    const NsBatch& b = t.b;
    if (!n || !d || !b.X || !b.xmean || !b.xstd || !b.XB || !t.PRED || !t.loss.YN || !t.loss.den || !t.loss.loss_rows || !t.loss.dP || b.B < 1) {
        set_error("net_forward_loss: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (d->nout != n->out_size) { set_error("net_forward_loss: loss for %d outputs, network has %d", d->nout, n->out_size); return LINNA_ERR_INVALID; }
    TRY(net_loss_current(n, d, stream, "net_forward_loss"));
    if (n->stream_loss != 1) { set_error("net_forward_loss: this network / loss does not run the whole-network kernel"); return LINNA_ERR_UNSUPPORTED; }
    if (n->L.size() > 1 && !t.fwd_ws) { set_error("net_forward_loss: workspace required"); return LINNA_ERR_INVALID; }
    const int rows = net_stream_rows(b.B);
    const float* packed = nullptr;
    TRY(stream_copy_refresh(n->packed_loss, n, rows, stream, &packed, NS_TRAIN_FWD, &n->loss_dn));
    const std::vector<NsOpBufs> ops = net_bufs(n, b.B, b.XB, b.ldxb, t.fwd_ws, t.PRED, t.ldp);
    TRY(launch_net_stream_train(net_layers(n, NS_TRAIN_FWD), packed, b, ops.data(), t.loss, n->loss_dn, rows, S(stream)));
    if (defer_post) return LINNA_OK;
    // the batch mean -- and, when the caller hands in its AdamW state, the step counter and bias corrections of the
    // update that will follow this step's backward (linna_adamw_step(prepared = 1))
    return launch_riders(train_riders(t), S(stream));
}
// Forward + loss + dX chain of a training step in ONE launch (net_stream.hip TRB), AdamW's step constants riding in it;
// the caller has found the mode TRAIN_MERGED or TRAIN_MERGED_BF16.
static int net_train_merged_impl(linna_net_t* n, const linna_loss_desc_t* d, const TrainStep& t, TrainMode mode, void* stream) {
    const NsBatch& b = t.b;
    if (!n || !d || !b.X || !b.xmean || !b.xstd || !b.XB || !t.PRED || !t.loss.YN || !t.loss.den || !t.loss.loss_rows || !t.loss.dP || !t.fwd_ws ||
        !t.bwd_ws || b.B < 1) {
        set_error("net_train_step: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (d->nout != n->out_size) { set_error("net_train_step: loss for %d outputs, network has %d", d->nout, n->out_size); return LINNA_ERR_INVALID; }
    const int rows = net_stream_rows(b.B);
    const TrainStreams ts = net_train_streams(n, mode);
    const float* packed = nullptr;
    TRY(stream_copy_refresh(*ts.fwd, n, rows, stream, &packed, ts.kind, &n->loss_dn));
    const std::vector<NsOpBufs> ops = net_bufs(n, b.B, b.XB, b.ldxb, t.fwd_ws, t.PRED, t.ldp, t.bwd_ws);   // (no input gradient)
    const NsPost post = train_riders(t);          // (only the step constants ride here: launch_net_stream_train_bwd)
    return launch_net_stream_train_bwd(net_layers(n, ts.kind), packed, b, ops.data(), t.loss, n->loss_dn, rows, S(stream),
                                       post.step ? &post : nullptr, mode == TRAIN_MERGED_BF16);
}
// (the loss descriptor's stream state, as net_forward_loss_impl establishes it)
static int net_train_ensure_loss(linna_net_t* n, const linna_loss_desc_t* d, void* stream) {
    if (!n || !d) { set_error("net_train_step: null argument"); return LINNA_ERR_INVALID; }
    return net_loss_current(n, d, stream, "net_train_step");
}
int linna_net_forward_loss(linna_net_t* n, const linna_loss_desc_t* d, const float* X, int ldx, const int* ROWS, int B,
                           const int* lg, const float* xmean, const float* xstd, float* XB, int ldxb, void* ws, float* PRED,
                           int ldp, const float* YN, int ldyn, const float* den, float inv_batch, float* loss_rows,
                           float* loss_mean, float* dPRED, int lddp, float* hyper, int* step_dev, float b1, float b2,
                           void* stream) try {
    if (!d) { set_error("net_forward_loss: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "net_forward_loss");
    const TrainStep t{{X, ldx, ROWS, B, lg, xmean, xstd, XB, ldxb}, {YN, ldyn, den, inv_batch, loss_rows, dPRED, lddp},
                      ws, nullptr, PRED, ldp, loss_mean, hyper, step_dev, b1, b2};
    return net_forward_loss_impl(n, d, t, stream, false);
} LINNA_CATCH_INT
// linna_net_train_step (linna_hip.h): linna_net_forward_loss followed by linna_net_backward(param_grads = 1) on the rows it
// gathered, the riders carried by the whole-network launches instead of a launch of their own between them.
int linna_net_train_step(linna_net_t* n, const linna_loss_desc_t* d, const float* X, int ldx, const int* ROWS, int B,
                         const int* lg, const float* xmean, const float* xstd, float* XB, int ldxb, void* fwd_ws, float* PRED,
                         int ldp, const float* YN, int ldyn, const float* den, float inv_batch, float* loss_rows,
                         float* loss_mean, float* dPRED, int lddp, void* bwd_ws, float* hyper, int* step_dev, float b1, float b2,
                         void* stream) try {
    if (!bwd_ws) { set_error("net_train_step: backward workspace required"); return LINNA_ERR_INVALID; }
    if (!d) { set_error("net_train_step: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "net_train_step");
    const TrainStep t{{X, ldx, ROWS, B, lg, xmean, xstd, XB, ldxb}, {YN, ldyn, den, inv_batch, loss_rows, dPRED, lddp},
                      fwd_ws, bwd_ws, PRED, ldp, loss_mean, hyper, step_dev, b1, b2};
    TRY(net_train_ensure_loss(n, d, stream));
    TRY(net_bf16_mode_check(n, B, "net_train_step"));
    const TrainMode mode = net_train_mode(n, B);
    if (mode == TRAIN_MERGED || mode == TRAIN_MERGED_BF16) {
        // two launches: forward + loss + dX chain, then every parameter gradient (the batch mean of the loss riding in it)
        TRY(net_train_merged_impl(n, d, t, mode, stream));
        const GemmPost gp{loss_rows, loss_mean ? B : 0, inv_batch, loss_mean};
        return net_train_backward(n, t, stream, BwdRiders{nullptr, nullptr, true, &gp});
    }
    // forward + loss, then the backward with the riders in its dX-chain launch (a launch of their own without one)
    TRY(net_forward_loss_impl(n, d, t, stream, true));
    const NsPost post = train_riders(t);
    return net_train_backward(n, t, stream, BwdRiders{post.out || post.step ? &post : nullptr});
} LINNA_CATCH_INT

int linna_net_train_launches(const linna_net_t* n, int B) try {
    if (!n || B < 1) { set_error("net_train_launches: bad arguments"); return LINNA_ERR_INVALID; }
    const TrainMode mode = net_train_mode(n, B);
    return mode == TRAIN_NONE ? 0 : mode == TRAIN_FWD_DX ? 3 : 2;
} LINNA_CATCH_INT
// The bf16 training step (linna_hip.h).  Checks first (no GPU), then the bf16 stream is allocated; its size depends on the
// network and the loss's width only, so a placeholder inverse covariance plans it before the loss is known.
int linna_net_set_train_precision(linna_net_t* n, int precision) try {
    if (!n) { set_error("net_set_train_precision: null handle"); return LINNA_ERR_INVALID; }
    TRY(check_precision(precision, "net_set_train_precision"));
    if (precision == LINNA_PRECISION_FP32) { n->train_prec = precision; n->as_state = -1; return LINNA_OK; }
    if (n->has_inskip) { set_error("net_set_train_precision: no bf16 training step for an input-skip network (it has no merged training step)"); return LINNA_ERR_UNSUPPORTED; }
    const NsDense dn = n->loss_dn.S ? n->loss_dn : NsDense{n->L.back().W, (int)ld4(n->out_size), nullptr, nullptr};
    const NsPlan plan = net_stream_plan(NS_TRAIN_STEP_BF16, n->L.data(), (int)n->L.size(), n->in_size, &dn);
    if (!plan.ok) { set_error("net_set_train_precision: no bf16 training step for this network: %s", plan.why ? plan.why : "not eligible"); return LINNA_ERR_UNSUPPORTED; }
    if (!n->packed_tbf.ready() || n->packed_tbf.floats != plan.packed_floats) {
        n->packed_tbf.release();
        if (n->packed_tbf.alloc(plan.packed_floats) != LINNA_OK) { set_error("net_set_train_precision: hipMalloc(bf16 training stream) failed"); return LINNA_ERR_HIP; }
    }
    n->train_prec = precision; n->as_state = -1;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_net_train_precision(const linna_net_t* n, int* out) try {
    if (!n || !out) { set_error("net_train_precision: null argument"); return LINNA_ERR_INVALID; }
    *out = n->train_prec;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_net_stream_state(const linna_net_t* n, int* fwd, int* dx, int* dx_input) try {
    if (!n) { set_error("net_stream_state: null network"); return LINNA_ERR_INVALID; }
    if (fwd) *fwd = n->stream_fwd;
    if (dx) *dx = n->stream_bwd[0];
    if (dx_input) *dx_input = n->stream_bwd[1];
    return LINNA_OK;
} LINNA_CATCH_INT

int linna_net_backward(linna_net_t* n, const float* X, int ldx, int B, void* fwd_ws, void* bwd_ws, const float* dOUT,
                       int lddo, float* dX, int lddx, int pg, void* stream) try {
    return net_backward_impl(n, X, ldx, B, fwd_ws, bwd_ws, dOUT, lddo, dX, lddx, pg, stream, BwdRiders{});
} LINNA_CATCH_INT

// ------------------------------------------------------------------ prior map
int linna_prior_map_fwd(linna_ctx_t*, const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1,
                        const float* a2, const int* lg, const float* xmean, const float* xstd, float* X, int ldx,
                        float* TH, int ldt, void* stream) try {
    if (ldx < nin || ldz < nin) { set_error("prior_map_fwd: leading dimension < nin"); return LINNA_ERR_INVALID; }
    return launch_prior_map_fwd(Z, ldz, B, nin, is_flat, a1, a2, lg, xmean, xstd, X, ldx, TH, ldt, S(stream));
} LINNA_CATCH_INT
int linna_prior_map_bwd(linna_ctx_t*, const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1,
                        const float* a2, const int* lg, const float* xstd, const float* dX, int lddx, float* dZ,
                        int lddz, void* stream) try {
    return launch_prior_map_bwd(Z, ldz, B, nin, is_flat, a1, a2, lg, xstd, dX, lddx, dZ, lddz, S(stream));
} LINNA_CATCH_INT

// ------------------------------------------------------------------ log-likelihood
int linna_gauss_loglike_diag(linna_ctx_t*, const float* D, int ldd, int B, int nout, const float* w, const float* Z,
                             int ldz, int nin, float T, float* out, void* stream) try {
    return launch_loglike_diag(D, ldd, B, nout, w, Z, ldz, nin, T, out, S(stream));
} LINNA_CATCH_INT
// cov: the inverse covariance S[nout][lds] -- or, factored, L with S = L L^T and the row-dot is |d L|^2 (linna_logprob_desc_t::Sfac)
static int loglike_dense_impl(const float* D, int ldd, int B, int nout, const NsDense& cov, const float* Z, int ldz, int nin, float T,
                              float* scratch, float* out, void* stream) {
    const int slots = gemm_slots(B, nout);
    GemmArgs a = gemm_zero();          // rows of (D S) dotted with D (or with themselves), no C store
    set_pair(a, 0, D, ldd, LAY_K, cov.S, cov.lds, LAY_MN, nout);
    a.M = B; a.N = nout; a.dotwith = D; a.lddot = ldd; a.dot_partial = scratch; a.dot_slots = slots;
    if (cov.factored) a.flags |= LINNA_GEMM_DOT_SELF;
    TRY(gemm_launch(a, S(stream)));
    return launch_loglike_finish(scratch, slots, slots, B, Z, ldz, nin, T, out, S(stream));
}
int linna_gauss_loglike_dense(linna_ctx_t*, const float* D, int ldd, int B, int nout, const float* Sm, int lds,
                              const float* Z, int ldz, int nin, float T, float* scratch, float* out, void* stream) try {
    return loglike_dense_impl(D, ldd, B, nout, NsDense{Sm, lds, nullptr, nullptr}, Z, ldz, nin, T, scratch, out, stream);
} LINNA_CATCH_INT

}  // extern "C"

// ------------------------------------------------------------------ serving pipeline
struct linna_logprob {
    linna_ctx* ctx;
    linna_net* net;
    linna_logprob_desc_t d;
    StreamCopy packed;                       // fragment-order weight streams (net_stream.hip), or not allocated
    bool grad_fused = false;                 // the streams also hold the backward segments (ReLU MLPs)
    StreamCopy packed_g2;                    // forward + dX chain down to the input in one stream (any network: residual blocks, ...)
    bool grad2 = false;
    bool g2_fits[3] = {true, true, true};    // packed_g2's program fits the LDS of the 16- / 8- / 4-row engine (net_stream_grad_fits)
    bool dense_fused = false;                // the streams end in the dense inverse covariance (output map folded in)
    bool fused_on = true;                    // LINNA_DISABLE_FUSED, read at creation
    int dense_tri = 2;                       // NsDense::tri, fixed when the object is created (the stream's size depends on it)
    NsDense dense() const { return NsDense{d.Sfac ? d.Sfac : d.S, d.lds, d.outmap.cscale, d.outmap.cshift, d.Sfac ? 1 : 0, dense_tri}; }
    int precision = LINNA_PRECISION_FP32;    // linna_logprob_set_precision
    StreamCopy packed_bf;                    // the bf16 weight streams (allocated when bf16 is first set, laid out lazily)
    bool bf16() const { return precision == LINNA_PRECISION_BF16; }
    int grad_precision = LINNA_PRECISION_FP32;   // linna_logprob_set_grad_precision (bf16 only on a bf16 handle)
    StreamCopy packed_gbf;                   // the bf16 forward + dX-chain streams (NS_GRAD_INPUT_BF16), allocated when it is first set
    bool dense_grad = false;                 // linna_logprob_set_dense_grad: a dense covariance's lnP and gradient in one launch (NS_GRAD_INPUT_DENSE)
    StreamCopy packed_gd;                    // ... its streams, allocated when it is first set
    bool gd_fits[3] = {false, false, false}; // ... and the engines (16 / 8 / 4 rows) whose LDS its program fits (net_stream_grad_dense_fits)
    NsKind kind() const { return bf16() ? NS_SERVE_BF16 : dense_fused ? NS_SERVE_DENSE : NS_SERVE; }   // the serving program
};

struct LpLayout { size_t x0, fwd, d, part, dh, bwd, dx, total; int slots; };
static LpLayout lp_layout(const linna_logprob* lp, int B, int with_grad) {
    LpLayout L;
    size_t off = 0;
    auto take = [&](size_t nfloats) { size_t o = off; off += (nfloats + 3) & ~(size_t)3; return o; };
    L.x0 = take((size_t)B * ld4(lp->d.nin));
    L.fwd = take(linna_net_fwd_ws_bytes(lp->net, B) / sizeof(float));
    L.d = take((size_t)B * ld4(lp->d.nout));
    L.slots = gemm_slots(B, lp->d.nout);
    L.part = take((size_t)B * L.slots);
    L.dh = L.bwd = L.dx = 0;
    if (with_grad) {
        L.dh = take((size_t)B * ld4(lp->d.nout));
        L.bwd = take(linna_net_bwd_ws_bytes(lp->net, B) / sizeof(float));
        L.dx = take((size_t)B * ld4(lp->d.nin));
    }
    L.total = off;
    return L;
}

// The copy the engine for `B` rows reads, re-laid if the weights moved since it was made; *rows: that engine.
static int lp_refresh_stream(linna_logprob* lp, int B, void* stream, const float** packed, int* rows) {
    *rows = net_stream_rows(B);
    const NsDense dn = lp->dense();
    return stream_copy_refresh(lp->bf16() ? lp->packed_bf : lp->packed, lp->net, *rows, stream, packed, lp->kind(),
                               lp->kind() == NS_SERVE_DENSE ? &dn : nullptr);
}
// THE output-map predicate: the map is complete (the exp map, cexp, has both halves) and, `with_likelihood`, this covariance
// rides in the launch (diagonal, or the last segment of a dense-fused stream).  0: no; 1: yes, the affine map; 2: yes, the exp map
static int lp_outmap_rides(const linna_logprob* lp, bool with_likelihood) {
    const linna_logprob_desc_t& d = lp->d;
    if (d.outmap.cexp && (!d.outmap.cpost || !d.outmap.cshift2)) return 0;
    if (with_likelihood && !d.w && !lp->dense_fused) return 0;
    return d.outmap.cexp ? 2 : 1;
}
// The descriptor's prior map and input transform, and its output map and diagonal likelihood, as the launchers take them.
// The dense program carries the output map and the covariance in its stream: it gets none of the latter; the second half
// of the exp output map is passed only when the map has one.
static NsInput lp_input(const linna_logprob_desc_t& d) { return NsInput{d.nin, d.is_flat, d.a1, d.a2, d.log10_flag, d.xmean, d.xstd}; }
static NsOutput lp_output(const linna_logprob* lp) {
    const linna_logprob_desc_t& d = lp->d;
    if (lp->kind() == NS_SERVE_DENSE) return NsOutput{nullptr, nullptr, nullptr, nullptr, nullptr, d.temperature};
    const bool ex = lp_outmap_rides(lp, false) == 2;
    return NsOutput{d.outmap.cscale, d.outmap.cshift, ex ? d.outmap.cpost : nullptr, ex ? d.outmap.cshift2 : nullptr, d.w, d.temperature};
}
// One launch of the serving program on the copy for `rows`, around a sampler move `mv` or with the fused gradient `gr` (or null)
static int lp_launch(const linna_logprob* lp, const float* packed, int rows, const NsRun& r, const NsMove* mv, const NsGrad* gr, void* stream) {
    const NsDense dn = lp->dense();
    return launch_net_stream(lp->kind(), net_layers(lp->net, lp->kind()), packed, r, lp_input(lp->d), lp_output(lp), mv, gr, rows,
                             lp->kind() == NS_SERVE_DENSE ? &dn : nullptr, S(stream));
}
// the serving stream of this handle's precision is there and switched on
static bool lp_stream_on(const linna_logprob* lp) { return lp->fused_on && (lp->bf16() ? lp->packed_bf.ready() : lp->packed.ready()); }
// Whether this log-probability runs the whole-network kernel around a sampler move (a bf16 handle runs the bf16 stream or
// nothing: where this refuses, the caller's fallback evaluates in bf16 too)
static bool lp_runs_fused_move(const linna_logprob* lp) { return lp_stream_on(lp) && lp_outmap_rides(lp, true) && lp->d.nin <= 64; }
// the likelihood of the residuals in the workspace as launches of their own: diagonal, or the dense row-dot
static int lp_likelihood(const linna_logprob* lp, const NsRun& r, float* w, const LpLayout& L, void* stream) {
    const linna_logprob_desc_t& d = lp->d;
    const int ldd = ld4(d.nout);
    if (d.w) return launch_loglike_diag(w + L.d, ldd, r.B, d.nout, d.w, r.Z, r.ldz, d.nin, d.temperature, r.lnP, S(stream));
    return loglike_dense_impl(w + L.d, ldd, r.B, d.nout, lp->dense(), r.Z, r.ldz, d.nin, d.temperature, w + L.part, r.lnP, stream);
}

// THE decision of what a call runs through, made once per call: the route, the engine where the route fixes it, for a refusal
// the code and the text behind the entry's name.  lp_forward and logprob_grad_impl switch on it, the queries read the same record.
enum LpRoute {
    LP_REFUSE,
    LP_EVAL_ONE,        // one whole-network launch, lnP from it (diagonal likelihood, dense-fused, every bf16 evaluation)
    LP_EVAL_FORWARD,    // the whole-network forward, then a likelihood launch of its own (dense covariance, not dense-fused)
    LP_EVAL_LAYERED,    // prior map, linna_net_forward, likelihood
    LP_GRAD_BF16,       // the bf16 one-launch program (packed_gbf)
    LP_GRAD_MLP,        // the MLP one-launch gradient of the serving stream (grad_fused)
    LP_GRAD_ANY,        // the any-network one-launch gradient (packed_g2) on the engine `rows`
    LP_GRAD_DENSE,      // the dense covariance's one-launch gradient (packed_gd; opt-in) on the engine `rows`
    LP_GRAD_LAYERED,    // layered forward, likelihood gradient, linna_net_backward, prior map's derivative
};
struct LpRouted { LpRoute route; int rows = 0; int err = LINNA_OK; const char* why = nullptr; };
// an evaluation; keep_activations: the layered gradient needs the forward's activations in the workspace
static LpRouted lp_eval_route(const linna_logprob* lp, bool keep_activations) {
    if (lp->bf16()) {
        // bf16 runs the whole-network kernel or nothing: never silently fp32
        if (!keep_activations && lp_stream_on(lp) && lp->d.w && lp_outmap_rides(lp, true)) return LpRouted{LP_EVAL_ONE};
        return LpRouted{LP_REFUSE, 0, LINNA_ERR_UNSUPPORTED,
                        "this bf16 log-probability cannot run the whole-network kernel here (LINNA_DISABLE_FUSED, or no diagonal likelihood)"};
    }
    if (keep_activations || !lp_stream_on(lp) || !lp_outmap_rides(lp, false)) return LpRouted{LP_EVAL_LAYERED};
    return LpRouted{lp_outmap_rides(lp, true) ? LP_EVAL_ONE : LP_EVAL_FORWARD};
}
// The engine the fp32 one-launch gradient (packed_g2) takes for B rows: the batch's own (or linna_engine_rows') where the
// program fits its LDS; 0: it does not -- the layered route, which was measured faster than a smaller engine's two rounds of
// workgroups (net_stream_grad_fits, net_program.hip)
static int lp_grad2_rows(const linna_logprob* lp, int B) {
    const int want = net_stream_rows(B);
    return lp->g2_fits[want == 16 ? 0 : want == 8 ? 1 : 2] ? want : 0;
}
// lnP and its gradient of B rows
static LpRouted lp_grad_route(const linna_logprob* lp, int B) {
    const linna_logprob_desc_t& d = lp->d;
    if (lp->bf16()) {
        if (lp->grad_precision != LINNA_PRECISION_BF16)
            return LpRouted{LP_REFUSE, 0, LINNA_ERR_UNSUPPORTED, "this log-probability is set to bf16, which serves lnP only (no bf16 gradient); set it back to fp32"};
        // the bf16 one-launch program or nothing: never a layered or fp32 form
        if (lp->fused_on && lp->packed_gbf.ready() && d.w && d.gscale && !d.outmap.cexp) return LpRouted{LP_GRAD_BF16, net_stream_rows(B)};
        return LpRouted{LP_REFUSE, 0, LINNA_ERR_UNSUPPORTED,
                        "this bf16 log-probability cannot run its one-launch gradient here (LINNA_DISABLE_FUSED, or no bf16 gradient stream)"};
    }
    if (d.outmap.cexp) return LpRouted{LP_REFUSE, 0, LINNA_ERR_UNSUPPORTED, "ypositive (exp) output map has no gradient path"};
    if (!d.gscale || (!d.w && !d.Ssym)) return LpRouted{LP_REFUSE, 0, LINNA_ERR_INVALID, "descriptor lacks gscale / Ssym"};
    if (lp_stream_on(lp) && lp->grad_fused && d.w) return LpRouted{LP_GRAD_MLP};
    if (lp->dense_grad && lp->fused_on && lp->packed_gd.ready() && !d.w && d.Sfac) {
        // the batch's own engine where the program fits it; otherwise the layered route, never a smaller engine (lp_grad2_rows)
        const int want = net_stream_rows(B);
        if (lp->gd_fits[want == 16 ? 0 : want == 8 ? 1 : 2]) return LpRouted{LP_GRAD_DENSE, want};
    }
    const int rows = lp->fused_on && lp->grad2 && lp->packed_g2.ready() && d.w ? lp_grad2_rows(lp, B) : 0;
    return rows ? LpRouted{LP_GRAD_ANY, rows} : LpRouted{LP_GRAD_LAYERED};
}

// lnP (and TH) of the rows `r` in the workspace w laid out as L, by the evaluation's route
static int lp_forward(linna_logprob* lp, const NsRun& r, float* w, const LpLayout& L, void* stream, bool keep_activations) {
    const linna_logprob_desc_t& d = lp->d;
    const int ldx = ld4(d.nin), ldd = ld4(d.nout), B = r.B;
    const LpRouted rt = lp_eval_route(lp, keep_activations);
    const float* packed = nullptr; int rows = 16;
    switch (rt.route) {
    case LP_EVAL_ONE:
        // whole-network kernel (net_stream.hip): prior map -> every layer -> output transform -> log-likelihood in ONE launch
        // (dense-fused: the output map is folded into the stream's last layer and the inverse covariance is its last segment)
        TRY(lp_refresh_stream(lp, B, stream, &packed, &rows));
        return lp_launch(lp, packed, rows, r, nullptr, nullptr, stream);
    case LP_EVAL_FORWARD:
        // ... the residuals into the workspace instead of lnP, for a likelihood launch of its own
        TRY(lp_refresh_stream(lp, B, stream, &packed, &rows));
        TRY(lp_launch(lp, packed, rows, NsRun{r.Z, r.ldz, B, nullptr, r.gate, r.TH, r.ldt, w + L.d, ldd}, nullptr, nullptr, stream));
        return lp_likelihood(lp, r, w, L, stream);
    case LP_EVAL_LAYERED:
        TRY(launch_prior_map_fwd(r.Z, r.ldz, B, d.nin, d.is_flat, d.a1, d.a2, d.log10_flag, d.xmean, d.xstd, w + L.x0, ldx, r.TH, r.ldt, S(stream)));
        TRY(linna_net_forward(lp->net, w + L.x0, ldx, B, w + L.fwd, w + L.d, ldd, &d.outmap, stream));
        return lp_likelihood(lp, r, w, L, stream);
    default: set_error("logprob: %s", rt.why); return rt.err;
    }
}

extern "C" {

int linna_logprob_create(linna_ctx_t* ctx, linna_net_t* net, const linna_logprob_desc_t* desc, linna_logprob_t** out) try {
    if (!net || !desc || !out) { set_error("logprob_create: null argument"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(desc, linna_logprob_desc_t, "logprob_create");
    if (desc->nin != net->in_size || desc->nout != net->out_size) {
        set_error("logprob_create: network is %d->%d, descriptor says %d->%d", net->in_size, net->out_size, desc->nin, desc->nout);
        return LINNA_ERR_INVALID;
    }
    if (!desc->w && !desc->S) { set_error("logprob_create: need S (dense) or w (diagonal)"); return LINNA_ERR_INVALID; }
    if (!(desc->temperature > 0.f)) { set_error("logprob_create: temperature must be > 0"); return LINNA_ERR_INVALID; }
    linna_logprob* lp = new linna_logprob{ctx, net, *desc};
    lp->dense_tri = net_stream_dense_tri(-1);
    lp->fused_on = !env_is("LINNA_DISABLE_FUSED", '1');     // 1: no whole-network kernel
    const NsDense dn = lp->dense();
    const bool want_dense = !desc->w && desc->S && !desc->outmap.cexp && !env_is("LINNA_DENSE_FUSED", '0');
    const NsPlan dense = want_dense ? net_stream_plan(NS_SERVE_DENSE, net->Lfull.data(), (int)net->Lfull.size(), net->in_size, &dn)
                                    : NsPlan{false, 0, false, nullptr};
    const NsPlan serve = net_stream_plan(NS_SERVE, net->Lfull.data(), (int)net->Lfull.size(), net->in_size);
    if (dense.ok) {
        lp->dense_fused = true;
        if (lp->packed.alloc(dense.packed_floats) != LINNA_OK) {
            set_error("logprob_create: hipMalloc(weight stream) failed");
            delete lp; return LINNA_ERR_HIP;
        }
    } else if (serve.ok) {
        lp->grad_fused = serve.grad_ok && !desc->outmap.cexp && !env_is("LINNA_DISABLE_FUSED_GRAD", '1');
        if (lp->packed.alloc(serve.packed_floats) != LINNA_OK) {
            set_error("logprob_create: hipMalloc(weight stream) failed");
            delete lp; return LINNA_ERR_HIP;
        }
    }
    // lnP + gradient in one launch for the networks the MLP-only fused gradient does not cover (residual blocks, SPLIT
    // segments): forward program + dX chain in one weight stream, gates from the activations the same launch stored
    if (!lp->grad_fused && desc->w && desc->gscale && !desc->outmap.cexp && !net->has_inskip && !env_is("LINNA_DISABLE_FUSED_GRAD", '1')) {
        const NsPlan g2 = net_stream_plan(ns_grad_kind(net->L.data(), (int)net->L.size()), net->L.data(), (int)net->L.size(), net->in_size);
        if (g2.ok && lp->packed_g2.alloc(g2.packed_floats) == LINNA_OK) lp->grad2 = true;
        // (fitted per engine once, here: wide outputs may not fit the LDS of the 16-row one)
        for (int e = 0; e < 3; ++e) lp->g2_fits[e] = net_stream_grad_fits(net->L.data(), (int)net->L.size(), net->in_size, 16 >> e);
    }
    *out = lp;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_logprob_destroy(linna_logprob_t* lp) try {
    if (lp) { lp->packed.release(); lp->packed_g2.release(); lp->packed_bf.release(); lp->packed_gbf.release(); lp->packed_gd.release(); }
    delete lp;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_weights_changed(linna_ctx_t*) try { g_weights_epoch.fetch_add(1); return LINNA_OK; } LINNA_CATCH_INT
// The opt-in bf16 serving engine.  Checks first (no GPU needed), then the bf16 streams are allocated here -- outside any
// graph capture -- and laid out by the first launch that reads them, like the fp32 copy (weight epoch).
int linna_logprob_set_precision(linna_logprob_t* lp, int precision) try {
    if (!lp) { set_error("logprob_set_precision: null handle"); return LINNA_ERR_INVALID; }
    TRY(check_precision(precision, "logprob_set_precision"));
    if (precision == LINNA_PRECISION_FP32) { lp->precision = precision; lp->grad_precision = LINNA_PRECISION_FP32; return LINNA_OK; }
    const linna_net* n = lp->net;
    if (!lp->d.w) { set_error("logprob_set_precision: bf16 needs a diagonal likelihood (a dense covariance is served in fp32 only)"); return LINNA_ERR_UNSUPPORTED; }
    const NsPlan bf = net_stream_plan(NS_SERVE_BF16, n->Lfull.data(), (int)n->Lfull.size(), n->in_size);
    if (!bf.ok) {
        set_error("logprob_set_precision: no bf16 engine for this network: %s", bf.why ? bf.why : "not eligible");
        return LINNA_ERR_UNSUPPORTED;
    }
    if (!lp->packed_bf.ready() && lp->packed_bf.alloc(bf.packed_floats) != LINNA_OK) {
        set_error("logprob_set_precision: hipMalloc(bf16 weight stream) failed");
        return LINNA_ERR_HIP;
    }
    lp->precision = precision;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_logprob_precision(const linna_logprob_t* lp, int* out) try {
    if (!lp || !out) { set_error("logprob_precision: null argument"); return LINNA_ERR_INVALID; }
    *out = lp->precision;
    return LINNA_OK;
} LINNA_CATCH_INT
// The second opt-in of a bf16 handle: lnP and its gradient from the bf16 one-launch program.  Checks first (no GPU needed),
// then the third stream copy is allocated here and laid out by the first launch that reads it (weight epoch).
int linna_logprob_set_grad_precision(linna_logprob_t* lp, int precision) try {
    if (!lp) { set_error("logprob_set_grad_precision: null handle"); return LINNA_ERR_INVALID; }
    TRY(check_precision(precision, "logprob_set_grad_precision"));
    if (precision == LINNA_PRECISION_FP32) { lp->grad_precision = precision; return LINNA_OK; }
    if (!lp->bf16()) {
        set_error("logprob_set_grad_precision: a bf16 gradient needs a bf16 handle (linna_logprob_set_precision first): lnP has one surface per handle");
        return LINNA_ERR_INVALID;
    }
    const linna_net* n = lp->net;
    if (lp->d.outmap.cexp) { set_error("logprob_set_grad_precision: no bf16 gradient: the ypositive (exp) output map has no gradient path"); return LINNA_ERR_UNSUPPORTED; }
    if (!lp->d.w || !lp->d.gscale) { set_error("logprob_set_grad_precision: no bf16 gradient: it needs a diagonal likelihood with gscale"); return LINNA_ERR_UNSUPPORTED; }
    const NsPlan g = net_stream_plan(NS_GRAD_INPUT_BF16, n->Lfull.data(), (int)n->Lfull.size(), n->in_size);
    if (!g.ok) {
        set_error("logprob_set_grad_precision: no bf16 gradient for this network: %s", g.why ? g.why : "not eligible");
        return LINNA_ERR_UNSUPPORTED;
    }
    if (!lp->packed_gbf.ready() && lp->packed_gbf.alloc(g.packed_floats) != LINNA_OK) {
        set_error("logprob_set_grad_precision: hipMalloc(bf16 gradient weight stream) failed");
        return LINNA_ERR_HIP;
    }
    lp->grad_precision = precision;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_logprob_grad_precision(const linna_logprob_t* lp, int* out) try {
    if (!lp || !out) { set_error("logprob_grad_precision: null argument"); return LINNA_ERR_INVALID; }
    *out = lp->grad_precision;
    return LINNA_OK;
} LINNA_CATCH_INT
// The opt-in one-launch gradient of a dense covariance.  Checks first (no GPU needed), then the stream copy is allocated here
// -- outside any graph capture -- and laid out by the first launch that reads it (weight epoch).
int linna_logprob_set_dense_grad(linna_logprob_t* lp, int on) try {
    if (!lp) { set_error("logprob_set_dense_grad: null handle"); return LINNA_ERR_INVALID; }
    if (on != 0 && on != 1) { set_error("logprob_set_dense_grad: %d (0 layered, 1 one launch)", on); return LINNA_ERR_INVALID; }
    if (!on) { lp->dense_grad = false; return LINNA_OK; }
    const linna_net* n = lp->net;
    const linna_logprob_desc_t& d = lp->d;
    if (lp->bf16()) { set_error("logprob_set_dense_grad: a bf16 handle has no dense-covariance gradient (fp32 only)"); return LINNA_ERR_UNSUPPORTED; }
    if (d.w) { set_error("logprob_set_dense_grad: the covariance is diagonal: its gradient is one launch already where the network has the program"); return LINNA_ERR_UNSUPPORTED; }
    if (d.outmap.cexp) { set_error("logprob_set_dense_grad: the ypositive (exp) output map has no gradient path"); return LINNA_ERR_UNSUPPORTED; }
    if (!d.Sfac) {
        set_error("logprob_set_dense_grad: no factored inverse covariance (Sfac): it is not positive definite, or LINNA_DENSE_FACTORED=0");
        return LINNA_ERR_UNSUPPORTED;
    }
    if (n->has_inskip) { set_error("logprob_set_dense_grad: an input-skip network has no one-launch gradient"); return LINNA_ERR_UNSUPPORTED; }
    const NsDense dn = lp->dense();
    const NsPlan g = net_stream_plan(NS_GRAD_INPUT_DENSE, n->L.data(), (int)n->L.size(), n->in_size, &dn);
    if (!g.ok) {
        set_error("logprob_set_dense_grad: no one-launch dense gradient for this network: %s", g.why ? g.why : "not eligible");
        return LINNA_ERR_UNSUPPORTED;
    }
    if (!lp->packed_gd.ready() && lp->packed_gd.alloc(g.packed_floats) != LINNA_OK) {
        set_error("logprob_set_dense_grad: hipMalloc(dense gradient weight stream) failed");
        return LINNA_ERR_HIP;
    }
    for (int e = 0; e < 3; ++e) lp->gd_fits[e] = net_stream_grad_dense_fits(n->L.data(), (int)n->L.size(), n->in_size, &dn, 16 >> e);
    lp->dense_grad = true;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_logprob_dense_grad(const linna_logprob_t* lp, int* out) try {
    if (!lp || !out) { set_error("logprob_dense_grad: null argument"); return LINNA_ERR_INVALID; }
    *out = lp->dense_grad ? 1 : 0;
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_program_describe_grad_dense(const linna_layer_t* layers, int nlayers, int in_size, int nout, int tri, int rows, char* buf, size_t n) try {
    if (!layers || nlayers < 1 || !buf || !n || nout < 1 || tri < 0 || tri > 2) { set_error("program_describe_grad_dense: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "program_describe_grad_dense"));
    if (layers[nlayers - 1].N != nout) { set_error("program_describe_grad_dense: %d columns for a network of %d outputs", nout, layers[nlayers - 1].N); return LINNA_ERR_INVALID; }
    // (pointers are only compared, never read: placeholders stand for the factor and the folded output map)
    static float dummy[2];
    const NsDense dn{dummy, (nout + 3) & ~3, dummy + 1, dummy + 1, 1, tri};
    return net_stream_describe(NS_GRAD_INPUT_DENSE, layers, nlayers, in_size, &dn, rows, buf, n);
} LINNA_CATCH_INT
int linna_program_describe_grad_bf16(const linna_layer_t* layers, int nlayers, int in_size, int rows, char* buf, size_t n) try {
    if (!layers || nlayers < 1 || !buf || !n) { set_error("program_describe_grad_bf16: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "program_describe_grad_bf16"));
    return net_stream_describe(NS_GRAD_INPUT_BF16, layers, nlayers, in_size, nullptr, rows, buf, n);
} LINNA_CATCH_INT
int linna_program_describe(const linna_layer_t* layers, int nlayers, int in_size, int rows, int dense_nout, char* buf, size_t n) try {
    if (!layers || nlayers < 1 || !buf || !n) { set_error("program_describe: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "program_describe"));
    // (pointers are only compared, never read: a placeholder stands for the dense inverse covariance)
    static float dummy;
    if (dense_nout == -1) return net_stream_describe(ns_grad_kind(layers, nlayers), layers, nlayers, in_size, nullptr, rows, buf, n);   // the one-launch gradient's program
    const int dn_cols = dense_nout < -1 ? -dense_nout : dense_nout;         // < -1: the factored form (chi^2 = |d L|^2) of -dense_nout columns
    NsDense dn{&dummy, (dn_cols + 3) & ~3, nullptr, nullptr, dense_nout < -1 ? 1 : 0, net_stream_dense_tri(-1)};
    if (dn_cols > 0) return net_stream_describe(NS_SERVE_DENSE, layers, nlayers, in_size, &dn, rows, buf, n);
    return net_stream_describe(NS_SERVE, layers, nlayers, in_size, nullptr, rows, buf, n);
} LINNA_CATCH_INT
int linna_serve_plain(int on) try {
    if (on < -1 || on > 1) { set_error("linna_serve_plain: %d (-1 query, 0 or 1)", on); return LINNA_ERR_INVALID; }
    return net_stream_serve_plain(on);
} LINNA_CATCH_INT
int linna_serve_plain_sched(int hand) try {
    if (hand < -1 || hand > 1) { set_error("linna_serve_plain_sched: %d (-1 query, 0 or 1)", hand); return LINNA_ERR_INVALID; }
    return net_stream_serve_plain_sched(hand);
} LINNA_CATCH_INT
int linna_serve_plain_trim(int on) try {
    if (on < -1 || on > 1) { set_error("linna_serve_plain_trim: %d (-1 query, 0 or 1)", on); return LINNA_ERR_INVALID; }
    return net_stream_serve_plain_trim(on);
} LINNA_CATCH_INT
int linna_program_trim(const linna_layer_t* layers, int nlayers, int in_size, int rows, char* buf, size_t n) try {
    if (!layers || nlayers < 1 || !buf || !n) { set_error("program_trim: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "program_trim"));
    return net_stream_trim_describe(layers, nlayers, in_size, rows, buf, n);
} LINNA_CATCH_INT
int linna_program_plain(const linna_layer_t* layers, int nlayers, int in_size, int rows, int dense_nout) try {
    if (!layers || nlayers < 1) { set_error("program_plain: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(check_layers(layers, nlayers, "program_plain"));
    if (dense_nout != 0) return 0;                                          // a dense segment: never plain
    return net_stream_program_plain(NS_SERVE, layers, nlayers, in_size, nullptr, rows) ? 1 : 0;
} LINNA_CATCH_INT
int linna_logprob_serve_plain(linna_logprob_t* lp, int B, int* out) try {
    if (!lp || !out || B < 1) { set_error("logprob_serve_plain: bad arguments"); return LINNA_ERR_INVALID; }
    // linna_logprob_eval's own route, and for the one launch that ends in lnP the launcher's own decision
    static float lnP;                                       // (stands for the caller's: only tested for null)
    *out = lp_eval_route(lp, false).route == LP_EVAL_ONE &&
           net_stream_takes_plain(lp->kind(), net_layers(lp->net, lp->kind()), lp_output(lp), NsRun{nullptr, 0, B, &lnP}, nullptr, nullptr,
                                  net_stream_rows(B), nullptr);
    return LINNA_OK;
} LINNA_CATCH_INT
int linna_dense_tri(int mode) try {
    if (mode < -1 || mode > 2) { set_error("linna_dense_tri: %d (-1 query, 0, 1 or 2)", mode); return LINNA_ERR_INVALID; }
    return net_stream_dense_tri(mode);
} LINNA_CATCH_INT
// which launches of linna_slice_half_step are folded into their neighbours (bit 0: the one stepping-out round's logic into
// the first shrinking round; bit 1: the set-up into the first evaluation's prologue; A/B switch, results identical either way)
static std::atomic<int> g_slice_fusion{7};
static bool slice_derive_enabled() { return (g_slice_fusion.load() & 1) != 0; }
int linna_slice_fusion(int mode) try {
    if (mode < -1 || mode > 7) { set_error("linna_slice_fusion: %d (-1 query, or a mask of bits 0-2)", mode); return LINNA_ERR_INVALID; }
    return mode < 0 ? g_slice_fusion.load() : g_slice_fusion.exchange(mode);
} LINNA_CATCH_INT
int linna_engine_rows(int rows) try {
    const int prev = net_stream_force_rows(rows);
    if (prev < 0) { set_error("linna_engine_rows: %d (0, 4, 8 or 16)", rows); return LINNA_ERR_INVALID; }
    // the packed-stream copies are cached per (16-row | small-batch) layout, not per engine: whatever was laid out under the
    // previous setting is re-laid before the next launch
    if (prev != rows) g_weights_epoch.fetch_add(1);
    return prev;
} LINNA_CATCH_INT
size_t linna_logprob_ws_bytes(const linna_logprob_t* lp, int B, int with_grad) try {
    return (lp_layout(lp, B, with_grad).total + 16) * sizeof(float);
} LINNA_CATCH_SIZE

int linna_logprob_eval(linna_logprob_t* lp, const float* Z, int ldz, int B, void* ws, float* lnP, float* TH, int ldt,
                       void* stream) try {
    if (!lp || !Z || !ws || !lnP || B < 1) { set_error("logprob_eval: bad arguments"); return LINNA_ERR_INVALID; }
    return lp_forward(lp, NsRun{Z, ldz, B, lnP, nullptr, TH, ldt}, static_cast<float*>(ws), lp_layout(lp, B, 0), stream, false);
} LINNA_CATCH_INT

int linna_logprob_eval_if(linna_logprob_t* lp, const float* Z, int ldz, int B, void* ws, float* lnP, float* TH, int ldt,
                          const int* gate, void* stream) try {
    if (!lp || !Z || !ws || !lnP || B < 1) { set_error("logprob_eval_if: bad arguments"); return LINNA_ERR_INVALID; }
    return lp_forward(lp, NsRun{Z, ldz, B, lnP, gate, TH, ldt}, static_cast<float*>(ws), lp_layout(lp, B, 0), stream, false);
} LINNA_CATCH_INT

// the first shrinking round behind one stepping-out round: what the evaluation needs to place its own trials (NsArgs::sl_*)
struct SliceDerive { const float* Z0; const float* L; const float* R; const float* Ze; int m, nt; uint64_t seed; const int* step_dev; int stream_id; const int* flags; };
// the walkers of a half step and their directions: trial point (j, k) = coords[S_idx[k]] + w[j * ns + k] * DIR[k]
struct SlicePoints { const float* coords; int ldc, ndim; const int* S_idx; int ns; const float* DIR; int ldd; };
// lnP[nrep * ns] at the trial points of weights w[nrep * ns], formed in the launch's prologue.
// `list` / `count` / `mul`: only the trial points list[0 .. count[0] * mul) are evaluated (device-side count; the launch is
// sized for all nrep * ns); `b_engine`: the batch size the engine is chosen for (the expected number of live rows);
// `sd` / `sb`: this evaluation derives its own trials (SliceDerive) / sets the half step up (SliceBegin)
static int lp_eval_slice_points(linna_logprob_t* lp, const SlicePoints& pt, const float* w, int nrep, float* lnP, const int* gate,
                                const int* list, const int* count, int mul, int b_engine, void* stream, const SliceDerive* sd = nullptr,
                                const SliceBegin* sb = nullptr) {
    if (!lp || !pt.coords || !pt.S_idx || !pt.DIR || !w || !lnP || pt.ns < 1 || nrep < 1) {
        set_error("logprob_eval_slice_points: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (pt.ndim != lp->d.nin) { set_error("logprob_eval_slice_points: ndim %d, log-probability has %d parameters", pt.ndim, lp->d.nin); return LINNA_ERR_INVALID; }
    if (!lp_runs_fused_move(lp)) {
        set_error("logprob_eval_slice_points: this log-probability does not run the whole-network kernel");
        return LINNA_ERR_UNSUPPORTED;          // the caller falls back to linna_slice_points + linna_logprob_eval_if
    }
    const float* packed = nullptr; int rows = 16;
    TRY(lp_refresh_stream(lp, b_engine > 0 ? b_engine : nrep * pt.ns, stream, &packed, &rows));
    NsMove mv{const_cast<float*>(pt.coords), pt.ldc, nullptr, pt.S_idx, w, 0, list, pt.ns, 0ull, count, mul, 0, 0.f, nullptr, 1};
    mv.sb = sb;
    if (sd) {
        mv.sl_Z0 = sd->Z0; mv.sl_L = sd->L; mv.sl_R = sd->R; mv.sl_Zt = sd->Ze; mv.sl_m = sd->m; mv.sl_nt = sd->nt;
        mv.sl_seed = sd->seed; mv.sl_step = sd->step_dev; mv.sl_stream = sd->stream_id; mv.sl_flags = sd->flags;
    }
    return lp_launch(lp, packed, rows, NsRun{pt.DIR, pt.ldd, nrep * pt.ns, lnP, gate}, &mv, nullptr, stream);
}
int linna_logprob_eval_slice_points(linna_logprob_t* lp, const float* coords, int ldc, int ndim, const int* S_idx, int ns,
                                    const float* DIR, int ldd, const float* w, int nrep, float* lnP, const int* gate,
                                    void* stream) try {
    return lp_eval_slice_points(lp, SlicePoints{coords, ldc, ndim, S_idx, ns, DIR, ldd}, w, nrep, lnP, gate, nullptr, nullptr, 0, 0, stream);
} LINNA_CATCH_INT

// One half step of the ensemble slice sampler (zeus behind sampler.py:728-735) in ONE call: the differential-move directions
// and slice heights, `nexp_rounds` speculative stepping-out rounds of `m_sched[r]` bracket ends per side, `nshr_rounds`
// shrinking rounds of `nt_sched[r]` trials with the commit in the last one -- 1 + 2 (nexp_rounds + nshr_rounds) launches, none of which the host waits for.
// Every evaluation is the whole-network kernel with the trial points formed in its prologue (never written to memory);
// rounds behind the one that finished the last walker are gated off on the device.
int linna_slice_half_step(linna_logprob_t* lp, float* coords, int ldc, int ndim, float* logp, const int* S_idx, int ns,
                          const float* ccoords, int ldcc, const int* C_idx, int nc, const float* mu, uint64_t seed,
                          int* step_dev, int half, const int* m_sched, int nexp_rounds, const int* nt_sched, int nshr_rounds,
                          float* DIR, int ldd, float* state, int* flags, float* W, float* Wd, float* Zt, int* list, int* counters,
                          int zero_totals, int bump_step, const int* expect_rows, int maxsteps, void* stream) try {
    if (!lp || !coords || !logp || !S_idx || !ccoords || !C_idx || !mu || !step_dev || !DIR || !state || !flags || !W || !Wd ||
        !Zt || !list || !counters || ns < 1 || nc < 2 || !m_sched || !nt_sched || nexp_rounds < 1 || nshr_rounds < 1 || (half != 0 && half != 1)) {
        set_error("slice_half_step: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (maxsteps < 1) { set_error("slice_half_step: maxsteps %d < 1", maxsteps); return LINNA_ERR_INVALID; }
    // (a round's bracket ends, 32 per side, and trials are held in one wave's lanes by the logic kernels: common.h)
    for (int r = 0; r < nexp_rounds; ++r)
        if (m_sched[r] < 1 || m_sched[r] > 32) { set_error("slice_half_step: m_sched[%d] = %d (1 to 32 bracket ends per side)", r, m_sched[r]); return LINNA_ERR_INVALID; }
    for (int r = 0; r < nshr_rounds; ++r)
        if (nt_sched[r] < 1 || nt_sched[r] > 64) { set_error("slice_half_step: nt_sched[%d] = %d (1 to 64 trials)", r, nt_sched[r]); return LINNA_ERR_INVALID; }
    if (ndim != lp->d.nin) { set_error("slice_half_step: ndim %d, log-probability has %d parameters", ndim, lp->d.nin); return LINNA_ERR_INVALID; }
    if (!lp_runs_fused_move(lp)) {
        set_error("slice_half_step: this log-probability does not run the whole-network kernel");
        return LINNA_ERR_UNSUPPORTED;          // the caller falls back to the round-by-round entries
    }
    float* const Z0 = state; float* const L = state + ns; float* const R = state + 2 * ns;
    float* const Wacc = state + 3 * ns; float* const Zacc = state + 4 * ns;
    hipStream_t st = S(stream);
    const SlicePoints pt{coords, ldc, ndim, S_idx, ns, DIR, ldd};
    // the set-up of the half step: a launch of its own, or done by the first evaluation in its prologue (SliceBegin)
    const bool begin_fused = (g_slice_fusion.load() & 2) != 0;
    const SliceBegin sb{logp, ccoords, ldcc, C_idx, nc, mu, seed, step_dev, half, m_sched[0], DIR, ldd, Z0, L, R, flags, counters,
                        nexp_rounds + nshr_rounds, zero_totals, maxsteps};
    if (!begin_fused)
        TRY(launch_slice_begin(sb, S_idx, ns, ndim, W, st));
    int slot = 4;
    // ONE stepping-out round (small ensembles): its logic kernel is not launched -- the first shrinking round's evaluation
    // derives its trial points from the stepping-out round's results in its prologue (NsArgs::sl_*), and the first shrinking
    // round's logic kernel does the bookkeeping of both.  The lnP of that round go to W (whose bracket ends are spent).
    const bool derive = slice_derive_enabled() && nexp_rounds == 1 && m_sched[0] <= 16 && nt_sched[0] <= 32 && nt_sched[0] <= 2 * m_sched[0];
    // rounds after the first evaluate only the walkers still active: the logic kernel of round r lists their trial points
    // (list[pos * nrep + j] = j ns + k, pos = the walker's rank among the active ones) and counts them in counters[slot];
    // round r + 1's launch is sized for all of them, runs the engine chosen for the expected number (`expect_rows`: what the
    // caller has seen in the usage counters of its earlier calls; without it a quarter of the walkers per round) and leaves
    // at the counted one.  Because only those walkers are evaluated, the later rounds can look
    // further ahead for nothing (m_sched / nt_sched grow) and the call needs few rounds.
    for (int r = 0; r < nexp_rounds; ++r, ++slot) {
        const int m = m_sched[r], m_next = r + 1 < nexp_rounds ? m_sched[r + 1] : 0;
        TRY(lp_eval_slice_points(lp, pt, W, 2 * m, Zt, nullptr, r > 0 ? list : nullptr, r > 0 ? counters + slot - 1 : nullptr, 2 * m,
                                 expect_rows && r > 0 ? std::max(1, expect_rows[r]) : std::max(1, (2 * m * ns) >> (2 * r)), stream, nullptr,
                                 r == 0 && begin_fused ? &sb : nullptr));
        if (!derive)
            TRY(launch_slice_expand_multi(Z0, Zt, L, R, S_idx, flags, ns, m, m_next, counters, slot, r > 0 ? slot - 1 : -1, W, Wd, list, seed,
                                          step_dev, 2 + half, nt_sched[0], st));
    }
    int trials = 0;
    for (int r = 0; r < nshr_rounds; ++r, ++slot) {
        const int nt = nt_sched[r], nt_next = r + 1 < nshr_rounds ? nt_sched[r + 1] : 0;
        trials += nt;
        const bool dv = derive && r == 0;
        SliceDerive sd{Z0, L, R, Zt, m_sched[0], nt, seed, step_dev, 2 + half, flags};
        TRY(lp_eval_slice_points(lp, pt, Wd, nt, dv ? W : Zt, nullptr, r > 0 ? list : nullptr, r > 0 ? counters + slot - 1 : nullptr, nt,
                                 expect_rows && r > 0 ? std::max(1, expect_rows[nexp_rounds + r]) : std::max(1, (nt * ns) >> (2 * r)), stream, dv ? &sd : nullptr));
        const bool last = r + 1 == nshr_rounds;         // the commit (and the step counter) ride in the last round's logic kernel
        SliceRound sr{Z0, dv ? W : Zt, L, R, S_idx, Wd, flags, Wacc, Zacc, ns, counters, slot, r > 0 ? slot - 1 : -1, nt, nt_next, trials, list,
                      seed, step_dev, 2 + half, last ? coords : nullptr, ldc, ndim, logp, DIR, ldd, last && bump_step ? 1 : 0,
                      Zt, dv ? m_sched[0] : 0, 4};
        TRY(launch_slice_shrink_multi(sr, st));
    }
    return LINNA_OK;
} LINNA_CATCH_INT

int linna_stretch_half_step(linna_logprob_t* lp, float* coords, int ldc, int ndim, float* logp, const int* S_idx, int ns,
                            const float* ccoords, int ldcc, const int* C_idx, int nc, uint64_t seed, const int* step_dev,
                            int step_offset, int stream_id, float a, int* naccept, void* stream) try {
    if (!lp || !coords || !logp || !S_idx || !ccoords || !C_idx || !step_dev || ns < 1 || nc < 1) {
        set_error("stretch_half_step: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (ndim != lp->d.nin) { set_error("stretch_half_step: ndim %d, log-probability has %d parameters", ndim, lp->d.nin); return LINNA_ERR_INVALID; }
    if (!lp_runs_fused_move(lp)) {
        set_error("stretch_half_step: this log-probability does not run the whole-network kernel");
        return LINNA_ERR_UNSUPPORTED;          // the caller falls back to propose / eval / accept
    }
    const float* packed = nullptr; int rows = 16;
    TRY(lp_refresh_stream(lp, ns, stream, &packed, &rows));
    NsMove mv{coords, ldc, logp, S_idx, ccoords, ldcc, C_idx, nc, seed, step_dev, step_offset, stream_id, a, naccept, 0};
    return lp_launch(lp, packed, rows, NsRun{nullptr, 0, ns, nullptr}, &mv, nullptr, stream);
} LINNA_CATCH_INT


int linna_stretch_run(linna_logprob_t* lp, float* coords, int ldc, int ndim, float* logp, int nw, const int* splits,
                      int split_stride, int nsteps, uint64_t seed, const int* step_dev, int step_offset, float a, int* naccept,
                      float* chain, float* logps, void* stream) try {
    if (!lp || !coords || !logp || !splits || !step_dev || nw < 2 || (nw & 1) || nsteps < 1 || split_stride < 0 ||
        (chain != nullptr) != (logps != nullptr)) {
        set_error("stretch_run: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (ndim != lp->d.nin) { set_error("stretch_run: ndim %d, log-probability has %d parameters", ndim, lp->d.nin); return LINNA_ERR_INVALID; }
    if (!lp_runs_fused_move(lp)) {
        set_error("stretch_run: this log-probability does not run the whole-network kernel");
        return LINNA_ERR_UNSUPPORTED;          // the caller loops over linna_stretch_half_step / the three-launch form
    }
    const int ns = nw / 2;
    const float* packed = nullptr; int rows = 16;
    TRY(lp_refresh_stream(lp, ns, stream, &packed, &rows));
    for (int i = 0; i < nsteps; ++i) {
        const int* sp = splits + (size_t)i * split_stride;
        for (int h = 0; h < 2; ++h) {
            NsMove mv{coords, ldc, logp, sp + h * ns, coords, ldc, sp + (1 - h) * ns, ns, seed, step_dev, step_offset + i, h, a, naccept, 0};
            if (chain) { mv.chain = chain + (size_t)i * nw * ndim; mv.lps = logps + (size_t)i * nw; }
            TRY(lp_launch(lp, packed, rows, NsRun{nullptr, 0, ns, nullptr}, &mv, nullptr, stream));
        }
    }
    return LINNA_OK;
} LINNA_CATCH_INT

}  // extern "C"

// the gradient's destination and, with `leap`, the leapfrog's kick and drift behind it (none: an NsLeap of nulls)
static NsGrad lp_grad_args(const linna_logprob_desc_t& d, float* G, int ldg, const NsLeap* leap) {
    return NsGrad{d.gscale, G, ldg, leap ? *leap : NsLeap{}};
}
// forward + dX chain down to the input in one launch on the stream copy `sc` (NS_GRAD_INPUT, or its bf16 form)
static int lp_launch_grad2(linna_logprob* lp, StreamCopy& sc, bool bf, const NsRun& r, const NsGrad& gr, int rows, void* stream) {
    const NsKind kind = bf ? NS_GRAD_INPUT_BF16 : ns_grad_kind(lp->net->L.data(), (int)lp->net->L.size());
    const float* packed = nullptr;
    TRY(stream_copy_refresh(sc, lp->net, rows, stream, &packed, kind));
    return launch_net_stream_grad2(net_layers(lp->net, kind), packed, r, lp_input(lp->d), lp_output(lp), gr, rows, S(stream), bf);
}
// the gradient's route is a refusal (the entries that enqueue other launches in front of the first gradient ask first: no
// refusal depends on the batch)
static int lp_grad_refused(const LpRouted& rt) {
    if (rt.route != LP_REFUSE) return LINNA_OK;
    set_error("logprob_grad: %s", rt.why);
    return rt.err;
}
// ---- what hmc.hip's whole-transition driver sees of this file (common.h)
int linna::logprob_nin(const linna_logprob_t* lp) { return lp->d.nin; }
int linna::logprob_grad_ready(const linna_logprob_t* lp) { return lp_grad_refused(lp_grad_route(lp, 1)); }
// lnP and its gradient at Z; `leap`: the leapfrog's kick and drift -- in the finish of the one-launch forms, as a launch of
// its own behind the others
int linna::logprob_grad_impl(linna_logprob_t* lp, const float* Z, int ldz, int B, void* ws, float* lnP, float* G, int ldg,
                             const NsLeap* leap, void* stream) {
    if (!lp || !Z || !ws || !lnP || !G || B < 1) { set_error("logprob_grad: bad arguments"); return LINNA_ERR_INVALID; }
    const LpRouted rt = lp_grad_route(lp, B);
    TRY(lp_grad_refused(rt));
    const linna_logprob_desc_t& d = lp->d;
    const NsGrad gr = lp_grad_args(d, G, ldg, leap);
    const NsRun r{Z, ldz, B, lnP};
    switch (rt.route) {
    case LP_GRAD_BF16: return lp_launch_grad2(lp, lp->packed_gbf, true, r, gr, rt.rows, stream);
    case LP_GRAD_MLP: {
        // lnP and d lnP / d z in ONE launch: forward segments, turnaround, backward segments over W^T (net_stream.hip)
        const float* packed = nullptr; int rows = 16;
        TRY(lp_refresh_stream(lp, B, stream, &packed, &rows));
        return lp_launch(lp, packed, rows, r, nullptr, &gr, stream);
    }
    case LP_GRAD_DENSE: {
        // ... and for a dense covariance (opt-in): the output map and the factor L of S = L L^T ride in the stream, the
        // turnaround works in U = d L (net_stream.hip, net_stream_dense_kernel) -- some thirty launches otherwise
        const NsDense dn = lp->dense();
        const float* packed = nullptr;
        TRY(stream_copy_refresh(lp->packed_gd, lp->net, rt.rows, stream, &packed, NS_GRAD_INPUT_DENSE, &dn));
        return launch_net_stream_grad_dense(net_layers(lp->net, NS_GRAD_INPUT_DENSE), packed, r, lp_input(d), d.temperature, gr, rt.rows, dn, S(stream));
    }
    case LP_GRAD_ANY:
        // ONE launch for any network: forward segments (the signs the gates need kept as bits in LDS), turnaround, dX chain
        // down to the input, prior map's derivative (net_stream.hip, GRAD + STORE == 2) -- six launches otherwise
        return lp_launch_grad2(lp, lp->packed_g2, false, r, gr, rt.rows, stream);
    default: break;                                         // LP_GRAD_LAYERED, below
    }
    const LpLayout L = lp_layout(lp, B, 1);
    float* w = static_cast<float*>(ws);
    const int ldx = ld4(d.nin), ldd = ld4(d.nout);
    TRY(lp_forward(lp, r, w, L, stream, true));
    if (d.w) {
        TRY(launch_loglike_diag_grad(w + L.d, ldd, B, d.nout, d.w, d.gscale, d.temperature, w + L.dh, ldd, S(stream)));
    } else {   // dH = -(1/T) * (D Ssym) * gscale
        GemmArgs a = gemm_zero();
        set_pair(a, 0, w + L.d, ldd, LAY_K, d.Ssym, d.lds, LAY_MN, d.nout);
        a.M = B; a.N = d.nout; a.C = w + L.dh; a.ldc = ldd; a.alpha0 = -1.f / d.temperature; a.cscale = d.gscale;
        TRY(gemm_launch(a, S(stream)));
    }
    TRY(linna_net_backward(lp->net, w + L.x0, ldx, B, w + L.fwd, w + L.bwd, w + L.dh, ldd, w + L.dx, ldx, 0, stream));
    TRY(launch_prior_map_bwd(Z, ldz, B, d.nin, d.is_flat, d.a1, d.a2, d.log10_flag, d.xstd, w + L.dx, ldx, G, ldg, S(stream)));
    if (leap) return launch_hmc_kick_drift(B, d.nin, leap->mass, leap->ek, leap->ed, G, ldg, leap->P, leap->ldp, leap->Q, ldz, S(stream), leap->eps);
    return LINNA_OK;
}

extern "C" {

int linna_logprob_grad(linna_logprob_t* lp, const float* Z, int ldz, int B, void* ws, float* lnP, float* G, int ldg,
                       void* stream) try {
    return logprob_grad_impl(lp, Z, ldz, B, ws, lnP, G, ldg, nullptr, stream);
} LINNA_CATCH_INT
// Whether that call is ONE launch for B rows under the current linna_engine_rows (host only: logprob_grad_impl's own decision)
int linna_logprob_grad_launches(linna_logprob_t* lp, int B, int* out) try {
    if (!lp || !out || B < 1) { set_error("logprob_grad_launches: bad arguments"); return LINNA_ERR_INVALID; }
    const LpRoute route = lp_grad_route(lp, B).route;
    *out = route == LP_GRAD_BF16 || route == LP_GRAD_MLP || route == LP_GRAD_ANY || route == LP_GRAD_DENSE ? 1 : 0;
    return LINNA_OK;
} LINNA_CATCH_INT

// One leapfrog step's gradient, kick and drift (HMCSampler.py:35-49): lnP and G = d lnP / d z at Q, then P += eps_kick G and
// Q += eps_drift P / mass.  ONE launch where linna_logprob_grad is one (the kick and the drift ride in its finish).
int linna_logprob_grad_leapfrog(linna_logprob_t* lp, float* Q, int ldq, int B, void* ws, float* lnP, float* G, int ldg, float* P,
                                int ldp, const float* mass, float eps_kick, float eps_drift, void* stream) try {
    if (!P || !mass || !Q) { set_error("logprob_grad_leapfrog: bad arguments"); return LINNA_ERR_INVALID; }
    const NsLeap leap{P, ldp, Q, mass, eps_kick, eps_drift, nullptr};
    return logprob_grad_impl(lp, Q, ldq, B, ws, lnP, G, ldg, &leap, stream);
} LINNA_CATCH_INT

int linna_logprob_grad_leapfrog_eps(linna_logprob_t* lp, float* Q, int ldq, int B, void* ws, float* lnP, float* G, int ldg, float* P,
                                    int ldp, const float* mass, const float* EPS, float mul_kick, float mul_drift, void* stream) try {
    if (!P || !mass || !Q || !EPS) { set_error("logprob_grad_leapfrog_eps: bad arguments"); return LINNA_ERR_INVALID; }
    const NsLeap leap{P, ldp, Q, mass, mul_kick, mul_drift, EPS};
    return logprob_grad_impl(lp, Q, ldq, B, ws, lnP, G, ldg, &leap, stream);
} LINNA_CATCH_INT

// ------------------------------------------------------------------ training
// scratch layout for the loss entry points: DELTA[B][ld] | U[B][ld] | partial[B][slots]
static size_t loss_scratch_floats(int B, int nout) { return (size_t)B * (2 * (size_t)ld4(nout) + gemm_slots(B, nout)); }

static int chi2_partials(const linna_loss_desc_t* d, int mode, const float* PRED, int ldp, const float* Y, int ldy,
                         const int* ROWS, int B, float* scratch, bool keepU, hipStream_t st) {
    const int ld = ld4(d->nout), slots = gemm_slots(B, d->nout);
    float* DELTA = scratch;
    float* U = scratch + (size_t)B * ld;
    float* part = scratch + 2 * (size_t)B * ld;
    TRY(launch_loss_delta(mode, PRED, ldp, Y, ldy, ROWS, B, *d, DELTA, ld, st));
    GemmArgs a = gemm_zero();
    set_pair(a, 0, DELTA, ld, LAY_K, d->Cinv, d->ldc, LAY_MN, d->nout);
    a.M = B; a.N = d->nout; a.C = keepU ? U : nullptr; a.ldc = ld;
    a.dotwith = DELTA; a.lddot = ld; a.dot_partial = part; a.dot_slots = slots;
    return gemm_launch(a, st);
}

size_t linna_loss_scratch_bytes(int B, int nout) try { return (loss_scratch_floats(B, nout) + 16) * sizeof(float); } LINNA_CATCH_SIZE

int linna_chi2_md(linna_ctx_t*, const linna_loss_desc_t* d, const float* Y, int ldy, int nrows, float* scratch,
                  float* den, void* stream) try {
    if (!d) { set_error("chi2_md: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "chi2_md");
    const int slots = gemm_slots(nrows, d->nout);
    TRY(chi2_partials(d, 1, nullptr, 0, Y, ldy, nullptr, nrows, scratch, false, S(stream)));
    return launch_loss_rows(0, scratch + 2 * (size_t)nrows * ld4(d->nout), slots, slots, nrows, nullptr, nullptr,
                            0.5f * (float)d->nout, den, S(stream));
} LINNA_CATCH_INT

int linna_chi2_ratio_loss_fwd_bwd(linna_ctx_t* ctx, const linna_loss_desc_t* d, const float* PRED, int ldp, const float* Y,
                                  int ldy, const float* den, const int* ROWS, int B, float* scratch, float* loss_rows,
                                  float* loss_mean, float* dPRED, int lddp, float inv_batch, void* stream) try {
    if (!d) { set_error("chi2_ratio_loss_fwd_bwd: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "chi2_ratio_loss_fwd_bwd");
    const int ld = ld4(d->nout), slots = gemm_slots(B, d->nout);
    hipStream_t st = S(stream);
    if (ctx && d->nout <= 64 && lddp >= 0) {
        // five launches of 5-14 us each (delta, U = delta Cinv, row sums, mean, gradient) for 2 MFLOP: one kernel
        if (ctx->loss_fused < 0) ctx->loss_fused = env_is("LINNA_LOSS_FUSED", '0') ? 0 : 1;
        unsigned* const cnt = ctx->loss_fused == 1 ? ctx->counters : nullptr;     // (zeroed, self-resetting: linna_ctx_create)
        if (cnt)
            return launch_loss_fused_small(PRED, ldp, Y, ldy, ROWS, B, *d, den, inv_batch, loss_rows, loss_mean, dPRED, lddp,
                                           cnt, st);
    }
    TRY(chi2_partials(d, 0, PRED, ldp, Y, ldy, ROWS, B, scratch, dPRED != nullptr, st));
    TRY(launch_loss_rows(1, scratch + 2 * (size_t)B * ld, slots, slots, B, den, ROWS, 0.f, loss_rows, st));
    if (loss_mean) TRY(launch_sum_scale(loss_rows, B, inv_batch, loss_mean, st));
    if (dPRED) TRY(launch_loss_grad(scratch + (size_t)B * ld, ld, Y, ldy, ROWS, B, d->nout, d->data_norm, den, inv_batch, dPRED, lddp, st));
    return LINNA_OK;
} LINNA_CATCH_INT

int linna_val_rows(linna_ctx_t*, const linna_loss_desc_t* d, const float* PRED, int ldp, const float* Y, int ldy,
                   const float* den, int B, float* scratch, float* loss_rows, float* frac_rows, void* stream) try {
    if (!d) { set_error("val_rows: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "val_rows");
    const int ld = ld4(d->nout), slots = gemm_slots(B, d->nout);
    hipStream_t st = S(stream);
    TRY(chi2_partials(d, 0, PRED, ldp, Y, ldy, nullptr, B, scratch, false, st));
    TRY(launch_loss_rows(1, scratch + 2 * (size_t)B * ld, slots, slots, B, den, nullptr, 0.f, loss_rows, st));
    TRY(chi2_partials(d, 2, PRED, ldp, Y, ldy, nullptr, B, scratch, false, st));
    return launch_val_frac(scratch + 2 * (size_t)B * ld, slots, slots, B, den, frac_rows, st);
} LINNA_CATCH_INT

int linna_val_metrics(linna_ctx_t*, const float* loss_rows, const float* frac_rows, int n, const float* last_train_loss, float* out,
                      void* stream) try {
    if (!loss_rows || !frac_rows || !out || n < 1 || n > (1 << 16)) {
        set_error("val_metrics: bad arguments (1 <= n <= 65536 validation rows)"); return LINNA_ERR_INVALID;
    }
    return launch_val_metrics(loss_rows, frac_rows, n, last_train_loss, out, S(stream));
} LINNA_CATCH_INT

int linna_gather_xform(linna_ctx_t*, const float* X, int ldx, const int* ROWS, int B, int nin, const int* lg,
                       const float* xmean, const float* xstd, float* XB, int ldxb, void* stream) try {
    return launch_gather_xform(X, ldx, ROWS, B, nin, lg, xmean, xstd, XB, ldxb, S(stream));
} LINNA_CATCH_INT

int linna_adamw_step(linna_ctx_t*, float* p, const float* g, float* m, float* v, size_t n, float* hyper, int* step_dev,
                     float b1, float b2, float eps, int prepared, void* stream) try {
    if (!p || !g || !m || !v || !hyper || !step_dev) { set_error("adamw_step: null pointer"); return LINNA_ERR_INVALID; }
    g_weights_epoch.fetch_add(1);
    // The step counter and the bias corrections are a single-thread launch of their own (folding them into the update
    // with an arrival counter measured 5 us slower than the extra launch): in front of the update here, or -- `prepared`
    // -- already advanced by linna_net_forward_loss, in the launch that takes the batch mean of the loss.
    return launch_adamw(p, g, m, v, n, hyper, prepared ? nullptr : step_dev, b1, b2, eps, S(stream));
} LINNA_CATCH_INT

// The placement tables of the flat parameter buffer `p[n]` in the streams a step of B rows trains through
// (net_stream_adamw_args), cached; the mode they describe is left in net->as_mode.
static int net_ensure_as_args(linna_net_t* net, int B, const float* p, size_t n) {
    TRY(net_bf16_mode_check(net, B, "net_adamw_step"));
    const TrainMode mode = net_train_mode(net, B);
    const TrainStreams ts = net_train_streams(net, mode);
    if (mode == TRAIN_NONE || !ts.fwd->ready() || (ts.dx && !ts.dx->ready())) {
        set_error("the network does not train through the whole-network streams"); return LINNA_ERR_UNSUPPORTED;
    }
    const int rows = net_stream_rows(B), k = rows < 16 ? 1 : 0;
    if (net->as_state < 0 || net->as_params != p || net->as_n != n || net->as_k != k || net->as_mode != mode) {
        net->as_params = p; net->as_n = n; net->as_k = k; net->as_mode = mode;
        const int merged = mode == TRAIN_MERGED_BF16 ? 2 : mode == TRAIN_MERGED ? 1 : 0;      // (net_stream_adamw_args' name for the mode)
        net->as_state = net_stream_adamw_args(net->L.data(), (int)net->L.size(), net->in_size, rows, p, n, ts.fwd->buf[k], &net->loss_dn,
                                              ts.dx ? ts.dx->buf[k] : nullptr, &net->as_args, merged) == LINNA_OK ? 1 : 0;
        net->upd_state = -1;
    }
    return net->as_state == 1 ? LINNA_OK : LINNA_ERR_UNSUPPORTED;   // (the error text is net_stream_adamw_args')
}

// linna_net_adamw_step (linna_hip.h): AdamW over the flat parameter buffer AND the re-layout of the updated weights into the
// streams a training step of B rows reads, in ONE launch.
int linna_net_adamw_step(linna_net_t* net, int B, float* p, const float* g, float* m, float* v, size_t n, float* hyper,
                         int* step_dev, float b1, float b2, float eps, int prepared, void* stream) try {
    if (!net || !p || !g || !m || !v || !hyper || !step_dev || B < 1) { set_error("net_adamw_step: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(net_ensure_as_args(net, B, p, n));
    // the streams must hold the CURRENT weights and their constant parts before they are patched in place
    const int rows = net_stream_rows(B);
    const TrainStreams ts = net_train_streams(net, net->as_mode);
    const float* dummy = nullptr;
    TRY(stream_copy_refresh(*ts.fwd, net, rows, stream, &dummy, ts.kind, &net->loss_dn));
    if (ts.dx) TRY(stream_copy_refresh(*ts.dx, net, rows, stream, &dummy, NS_DX));
    if (!prepared) TRY(launch_adamw_prepare(hyper, step_dev, b1, b2, S(stream)));
    TRY(launch_adamw_streams(net->as_args, p, g, m, v, hyper, b1, b2, eps, S(stream), net->as_mode == TRAIN_MERGED_BF16));
    net_stamp_updated(net, net->as_mode, B, stream);
    return LINNA_OK;
} LINNA_CATCH_INT

// linna_net_train_step_update (linna_hip.h): linna_net_train_step with AdamW in the epilogue of its grouped parameter-gradient
// launch -- every 64 x 64 gradient tile updates its block of the weight matrix (and its moments) as soon as it exists and
// writes the updated block into the weight streams the next step reads.  LINNA_ERR_UNSUPPORTED before anything is launched.
int linna_net_train_step_update(linna_net_t* net, const linna_loss_desc_t* d, const float* X, int ldx, const int* ROWS, int B,
                                const int* lg, const float* xmean, const float* xstd, float* XB, int ldxb, void* fwd_ws, float* PRED,
                                int ldp, const float* YN, int ldyn, const float* den, float inv_batch, float* loss_rows,
                                float* loss_mean, float* dPRED, int lddp, void* bwd_ws, float* params, float* m, float* v,
                                size_t n, float* hyper, int* step_dev, float b1, float b2, float eps, void* stream) try {
    if (!net || !params || !m || !v || !hyper || !step_dev || !bwd_ws || B < 1) { set_error("net_train_step_update: bad arguments"); return LINNA_ERR_INVALID; }
    if (!d) { set_error("net_train_step_update: null loss descriptor"); return LINNA_ERR_INVALID; }
    CHECK_STRUCT(d, linna_loss_desc_t, "net_train_step_update");
    if (net->has_inskip) { set_error("net_train_step_update: input-skip network"); return LINNA_ERR_UNSUPPORTED; }
    const TrainStep t{{X, ldx, ROWS, B, lg, xmean, xstd, XB, ldxb}, {YN, ldyn, den, inv_batch, loss_rows, dPRED, lddp},
                      fwd_ws, bwd_ws, PRED, ldp, loss_mean, hyper, step_dev, b1, b2};
    TRY(net_train_ensure_loss(net, d, stream));
    TRY(net_bf16_mode_check(net, B, "net_train_step_update"));
    TRY(net_ensure_as_args(net, B, params, n));
    if (net->upd_state < 0 || net->upd_B != B) {
        // every parameter gradient of the step must be a problem of the grouped launch, and the gradient pointers of the layer
        // table must mirror the parameter buffer (same distance for every tensor)
        bool ok = net->ctx != nullptr;         // (the grouped launch needs a context)
        int nprob = 0;
        long long diff = 0; bool have = false;
        auto same = [&](const float* w, const float* g) { if (!w) return; if (!g) { ok = false; return; } if (!have) { diff = w - g; have = true; } else if (w - g != diff) ok = false; };
        auto prob = [&](int M, int N) {
            GemmArgs a = gemm_zero();
            a.npairs = 1; a.p[0].alay = LAY_MN; a.p[0].blay = LAY_MN; a.p[0].lda = ld4(M); a.p[0].ldb = ld4(N); a.p[0].K = B; a.M = M; a.N = N;
            if (!gemm_group_ok(a)) ok = false;
            ++nprob;
        };
        for (const linna_layer_t& l : net->L) {
            if (l.op == LINNA_OP_LINEAR) { prob(l.N, l.K); same(l.W, l.gW); same(l.b, l.gb); }
            else if (l.op == LINNA_OP_RESBLOCK) {
                prob(l.N, l.C); prob(l.C, l.K); if (l.Ws) prob(l.N, l.K);
                same(l.W1, l.gW1); same(l.b1, l.gb1); same(l.W2, l.gW2); same(l.b2, l.gb2); same(l.Ws, l.gWs);
            } else ok = false;
        }
        net->upd_state = (ok && nprob <= GEMM_UPD_MAX) ? 1 : 0;
        net->upd_B = B;
    }
    if (net->upd_state != 1) {
        set_error("net_train_step_update: a parameter gradient of this network falls outside the grouped launch%s", net_bf16(net) ? " (bf16 step)" : "");
        return LINNA_ERR_UNSUPPORTED;
    }
    const TrainMode mode = net->as_mode;
    const NetUpdate upd{params, m, v, hyper, b1, b2, eps, mode == TRAIN_MERGED_BF16};
    if (mode != TRAIN_FWD_DX) {
        // TWO launches: forward + loss + dX chain (AdamW's step constants riding in it), then every parameter gradient with the
        // optimiser in the tiles' epilogue (the batch mean of the loss riding in it)
        TRY(net_train_merged_impl(net, d, t, mode, stream));
        const GemmPost gp{loss_rows, loss_mean ? B : 0, inv_batch, loss_mean};
        TRY(net_train_backward(net, t, stream, BwdRiders{nullptr, &upd, true, &gp}));
    } else {
        TRY(net_forward_loss_impl(net, d, t, stream, true));
        const NsPost post = train_riders(t);
        TRY(net_train_backward(net, t, stream, BwdRiders{&post, &upd}));
    }
    net_stamp_updated(net, mode, B, stream);
    return LINNA_OK;
} LINNA_CATCH_INT

// ------------------------------------------------------------------ moves
int linna_stretch_propose(linna_ctx_t*, const float* coords, int ldc, int ndim, const int* S_idx, int ns,
                          const float* ccoords, int ldcc, const int* C_idx, int nc, uint64_t seed, const int* step_dev,
                          int stream_id, float a, float* Q, int ldq, float* factors, void* stream) try {
    if (ns < 1 || nc < 1) { set_error("stretch_propose: empty walker set"); return LINNA_ERR_INVALID; }
    return launch_stretch_propose(coords, ldc, ndim, S_idx, ns, ccoords, ldcc, C_idx, nc, seed, step_dev, stream_id, a, Q,
                                  ldq, factors, S(stream));
} LINNA_CATCH_INT
int linna_stretch_accept(linna_ctx_t*, float* coords, int ldc, int ndim, float* logp, const int* S_idx, int ns,
                         const float* Q, int ldq, const float* logp_new, const float* factors, uint64_t seed,
                         const int* step_dev, int stream_id, int* naccept, void* stream) try {
    return launch_stretch_accept(coords, ldc, ndim, logp, S_idx, ns, Q, ldq, logp_new, factors, seed, step_dev, stream_id, naccept, S(stream));
} LINNA_CATCH_INT
int linna_step_increment(linna_ctx_t*, int* step_dev, void* stream) try { return launch_step_increment(step_dev, S(stream)); } LINNA_CATCH_INT

int linna_slice_init(linna_ctx_t*, const float* logp, const int* S_idx, int ns, const float* cc, int ldcc, const int* C_idx,
                     int nc, int ndim, const float* mu, uint64_t seed, const int* step_dev, int stream_id, float* DIR,
                     int ldd, float* Z0, float* L, float* R, int* flags, int maxsteps, void* stream) try {
    if (ns < 1 || nc < 2) { set_error("slice_init: need >= 2 complementary walkers"); return LINNA_ERR_INVALID; }
    if (maxsteps < 1) { set_error("slice_init: maxsteps %d < 1", maxsteps); return LINNA_ERR_INVALID; }
    // the set-up kernel of linna_slice_half_step without its first round's bracket ends and its usage counters
    const SliceBegin sb{logp, cc, ldcc, C_idx, nc, mu, seed, step_dev, stream_id, 0, DIR, ldd, Z0, L, R, flags, nullptr, 0, 0, maxsteps};
    return launch_slice_begin(sb, S_idx, ns, ndim, nullptr, S(stream));
} LINNA_CATCH_INT
int linna_slice_points(linna_ctx_t*, const float* coords, int ldc, int ndim, const int* S_idx, int ns, const float* DIR,
                       int ldd, const float* w, float* Q, int ldq, int nrep, void* stream) try {
    if (nrep < 1) { set_error("slice_points: nrep < 1"); return LINNA_ERR_INVALID; }
    return launch_slice_points(coords, ldc, ndim, S_idx, ns, DIR, ldd, w, Q, ldq, nrep, S(stream));
} LINNA_CATCH_INT
int linna_slice_expand(linna_ctx_t*, const float* Z0, const float* ZL, const float* ZR, float* L, float* R, int* flags,
                       int ns, int* counters, int slot, void* stream) try {
    return launch_slice_expand(Z0, ZL, ZR, L, R, flags, ns, counters, slot, S(stream));
} LINNA_CATCH_INT
int linna_slice_draw(linna_ctx_t*, const float* L, const float* R, const int* S_idx, float* W, const int* flags, int ns,
                     uint64_t seed, const int* step_dev, int stream_id, int round, int ntrial, void* stream) try {
    if (ntrial < 1 || ntrial > 64) { set_error("slice_draw: ntrial %d (1 to 64)", ntrial); return LINNA_ERR_INVALID; }
    return launch_slice_draw(L, R, S_idx, W, flags, ns, seed, step_dev, stream_id, round, ntrial, S(stream));
} LINNA_CATCH_INT
int linna_slice_shrink(linna_ctx_t*, const float* Z0, const float* Zt, float* L, float* R, const float* W, int* flags,
                       float* Wacc, float* Zacc, int ns, int* counters, int slot, int ntrial, void* stream) try {
    if (ntrial < 1 || ntrial > 64) { set_error("slice_shrink: ntrial %d (1 to 64)", ntrial); return LINNA_ERR_INVALID; }
    return launch_slice_shrink(Z0, Zt, L, R, W, flags, Wacc, Zacc, ns, counters, slot, ntrial, S(stream));
} LINNA_CATCH_INT
int linna_slice_commit(linna_ctx_t*, float* coords, int ldc, int ndim, float* logp, const int* S_idx, int ns,
                       const float* DIR, int ldd, const float* Wacc, const float* Zacc, void* stream) try {
    return launch_slice_commit(coords, ldc, ndim, logp, S_idx, ns, DIR, ldd, Wacc, Zacc, S(stream));
} LINNA_CATCH_INT

}  // extern "C"
