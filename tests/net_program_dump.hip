// Dumps the whole-network kernel's planner (csrc/net_program.hip) as text, on a CPU: tests/test_net_program_host.py links
// this file with the planner object alone and compares every case with the expectation committed under tests/golden/.
//
// stdin, per case:
//   case <id> <NsKind> <rows> <in_size> <dense: 0 none, 1 unfactored, 2 factored> <tri> <nl>
//   <op> <K> <C> <N> <relu> <alpha> <W> <b> <W1> <b1> <W2> <b2> <Ws>          (nl lines; tensors as placeholder addresses)
// stdout, per case: the full dump, one "  "-indented line per record, then
//   == <id> | <describe-style summary> | <FNV-1a 64 of the dump>
#include "net_program.h"
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace linna {
static std::string g_error;
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_error = buf;
}
int check_hip(hipError_t e, const char*) { return e == hipSuccess ? LINNA_OK : LINNA_ERR_HIP; }
}  // namespace linna
using namespace linna;

static std::string g_out;
static void emit(const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_out += "  "; g_out += buf; g_out += "\n";
}
static float* fake(uint64_t a) { return reinterpret_cast<float*>(static_cast<uintptr_t>(a)); }

// the dense descriptor's placeholders, and the streams of the AdamW table
static const uint64_t DN_S = 0x70000000, DN_CSCALE = 0x70800000, DN_CSHIFT = 0x70900000;
static const uint64_t S_FWD = 0x100000000ull, S_DX = 0x200000000ull, PARAMS = 0x40000000;

struct Names { std::vector<std::pair<const float*, std::string>> v; };
static void name_layers(Names& nm, const std::vector<linna_layer_t>& L) {
    for (size_t i = 0; i < L.size(); ++i) {
        const linna_layer_t& l = L[i];
        const std::pair<const float*, const char*> f[] = {{l.W, "W"}, {l.b, "b"}, {l.W1, "W1"}, {l.b1, "b1"}, {l.W2, "W2"}, {l.b2, "b2"}, {l.Ws, "Ws"}};
        for (const auto& t : f) if (t.first) nm.v.push_back({t.first, "L" + std::to_string(i) + "." + t.second});
    }
    nm.v.push_back({fake(DN_S), "S"}); nm.v.push_back({fake(DN_CSCALE), "cscale"}); nm.v.push_back({fake(DN_CSHIFT), "cshift"});
}
static std::string nameof(const Names& nm, const float* p) {
    if (!p) return "-";
    for (const auto& t : nm.v) if (t.first == p) return t.second;
    return "?";
}
static std::string stream_off(const float* p) {
    if (!p) return "-";
    const uint64_t a = reinterpret_cast<uintptr_t>(p);
    return (a >= S_DX ? "dx+" : "fwd+") + std::to_string((a - (a >= S_DX ? S_DX : S_FWD)) / sizeof(float));
}

static void dump_program(const NsProgram& p, const Names& nm, int rows) {
    // what a caller reads of a program that is not eligible is net_stream_describe's header line
    emit("program ok %d G %d Gstride %d nseg_f %d LD %d kpad0 %d packed_floats %zu grad_ok %d", (int)p.ok, p.G, p.Gstride, p.nseg_f, p.LD,
         p.kpad0, p.packed_floats, (int)p.grad_ok);
    if (!p.ok) return;
    emit("nseg %zu nout %d bias_total %d mask_slots %d dense %d u_col %d u_same %d x0_keep %d side_f4 %zu bf %d f32seg %d dxi_ok %d train_ok %d",
         p.seg.size(), p.nout, p.bias_total, p.mask_slots, p.dense, p.u_col, p.u_same, p.x0_keep, p.side_f4, (int)p.bf, p.f32seg,
         (int)p.dxi_ok, (int)p.train_ok);
    emit("lds rows %d: %zu grad %zu; 16 rows: %zu grad %zu", rows, p.lds_for(rows, false), p.lds_for(rows, true), p.lds_for(NS_ROWS, false),
         p.lds_for(NS_ROWS, true));
    for (size_t i = 0; i < p.seg.size(); ++i) {
        const NsSeg& s = p.seg[i];
        const NsPackSeg& q = p.pack[i];
        emit("seg %zu op %d hidden %d type %d steps %d passes %d bias_off %d dst_col %d relu %d kslice %d zext %d ncg_log2 %d mask_store %d "
             "mask_apply %d x0_n %d x0_col %d kcl %d side_off %d stream_steps %d", i, p.seg_op[i], p.seg_hidden[i], s.type, s.steps, s.passes,
             s.bias_off, s.dst_col, s.relu, s.kslice, s.zext, s.ncg_log2, s.mask_store, s.mask_apply, s.x0_n, s.x0_col, s.kcl, s.side_off,
             ns_seg_steps(s));
        emit("pack %zu Wa %s lda %d Ka %d Kapad %d Wb %s ldb %d Kb %d alpha %.9g b %s bscale %.9g b2 %s b2scale %.9g N %d type %d steps %d "
             "passes %d bias_off %d bias_pad %d ncg %d transA %d transB %d rscale %s rshift %s kc %d side_off %d koff2 %d", i,
             nameof(nm, q.Wa).c_str(), q.lda, q.Ka, q.Kapad, nameof(nm, q.Wb).c_str(), q.ldb, q.Kb, q.alpha, nameof(nm, q.b).c_str(), q.bscale,
             nameof(nm, q.b2).c_str(), q.b2scale, q.N, q.type, q.steps, q.passes, q.bias_off, q.bias_pad, q.ncg, q.transA, q.transB,
             nameof(nm, q.rscale).c_str(), nameof(nm, q.rshift).c_str(), q.kc, q.side_off, q.koff2);
    }
}

static void dump_gates(const NsProgram& p, const std::vector<linna_layer_t>& L, int rows) {
    const NsGates g = ns_gates(p, L.data(), (int)L.size(), rows);
    emit("gates ok %d ncols %d lds0 %zu lds %zu", (int)g.ok, g.ncols, g.lds0, g.lds);
    for (size_t i = 0; i < p.seg.size(); ++i)              // (the loss segment stands for no layer: no columns to ask for)
        emit("gate %zu gbit %d mbit %d cols %d", i, g.gbit[i], g.mbit[i], p.seg_op[i] < (int)L.size() ? ns_seg_cols(p, L.data(), (int)i) : -1);
}

// the AdamW descriptor table over the same layers with their tensors back to back in one flat buffer
static void dump_adamw(std::vector<linna_layer_t> L, int in_size, int rows, const NsDense* dn, int merged) {
    uint64_t off = 0;
    auto next = [&](size_t nf) { float* p = fake(PARAMS + off * sizeof(float)); off += nf; return p; };
    auto mat = [&](int N, int K) { return next((size_t)N * ((K + 3) & ~3)); };
    auto vec = [&](int N) { return next((size_t)((N + 3) & ~3)); };
    for (linna_layer_t& l : L) {
        if (l.op == LINNA_OP_RESBLOCK) {
            l.W1 = mat(l.C, l.K); l.b1 = vec(l.C); l.W2 = mat(l.N, l.C); l.b2 = vec(l.N);
            if (l.Ws) l.Ws = mat(l.N, l.K);
        } else { l.W = mat(l.N, l.K); l.b = vec(l.N); }
    }
    Names nm; name_layers(nm, L);
    AsArgs a;
    g_error.clear();
    const int rc = net_stream_adamw_args(L.data(), (int)L.size(), in_size, rows, fake(PARAMS), (size_t)off, fake(S_FWD), dn, fake(S_DX), &a, merged);
    emit("adamw merged %d rc %d%s%s", merged, rc, rc ? " error: " : "", rc ? g_error.c_str() : "");
    if (rc != LINNA_OK) return;
    emit("adamw nr %d small %d nblocks %u", a.nr, a.small, a.nblocks);
    for (int i = 0; i < a.nr; ++i) {
        const AsRange& R = a.r[i];
        emit("range %d off4 %u n4 %u blk0 %u kind %d idx %d", i, R.off4, R.n4, R.blk0, (int)R.kind, (int)R.idx);
        if (R.kind == 1) {
            const AsBias& B = a.b[R.idx];
            emit("bias %d out %s scale %.9g N %d", (int)R.idx, stream_off(B.out).c_str(), B.scale, B.N);
            continue;
        }
        const AsMat& W = a.w[R.idx];
        emit("mat %d N %d ld %d", (int)R.idx, W.N, W.ld);
        for (int j = 0; j < 2; ++j) {
            const AsPlace& q = W.pl[j];
            emit("place %d out %s scale %.9g trans %d koff %d ncols %d type %d ncg %d steps %d G %d first0 %d first1 %d", j, stream_off(q.out).c_str(),
                 q.scale, q.trans, q.koff, q.ncols, q.type, q.ncg, q.steps, q.G, q.first0, q.first1);
        }
    }
}

static uint64_t fnv1a(const std::string& s) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    return h;
}

int main() {
    char id[128];
    int kind, rows, in_size, dense, tri, nl;
    while (scanf(" case %127s %d %d %d %d %d %d", id, &kind, &rows, &in_size, &dense, &tri, &nl) == 7) {
        std::vector<linna_layer_t> L((size_t)(nl > 0 ? nl : 0));
        for (linna_layer_t& l : L) {
            unsigned long long t[7];
            std::memset(&l, 0, sizeof l);
            l.struct_size = sizeof l;
            if (scanf("%d %d %d %d %d %f %llu %llu %llu %llu %llu %llu %llu", &l.op, &l.K, &l.C, &l.N, &l.relu, &l.alpha, &t[0], &t[1], &t[2], &t[3],
                      &t[4], &t[5], &t[6]) != 13) { fprintf(stderr, "%s: bad layer line\n", id); return 2; }
            l.W = fake(t[0]); l.b = fake(t[1]); l.W1 = fake(t[2]); l.b1 = fake(t[3]); l.W2 = fake(t[4]); l.b2 = fake(t[5]); l.Ws = fake(t[6]);
        }
        int nout = 0;                                         // the dense matrix spans the network output
        for (const linna_layer_t& l : L) if (l.op != LINNA_OP_INSKIP) nout = l.N;
        const NsKind k = (NsKind)kind;
        const bool serve = k == NS_SERVE_DENSE;              // (the serving program folds its output map; the loss has none)
        NsDense dn{fake(DN_S), (nout + 3) & ~3, serve ? fake(DN_CSCALE) : nullptr, serve ? fake(DN_CSHIFT) : nullptr, dense == 2 ? 1 : 0, tri};
        const NsDense* const dnp = dense ? &dn : nullptr;
        Names nm; name_layers(nm, L);
        g_out.clear();
        const NsProgramRef pref = ns_program(k, L.data(), nl, in_size, dnp, rows);
        const NsProgram& p = *pref;
        dump_program(p, nm, rows);
        const bool gated = k == NS_GRAD_INPUT || k == NS_TRAIN_STEP || k == NS_TRAIN_STEP_BF16;
        if (p.ok && gated && (k == NS_GRAD_INPUT ? p.dxi_ok : p.train_ok)) dump_gates(p, L, rows);
        const NsPlan plan = net_stream_plan(k, L.data(), nl, in_size, dnp);
        emit("plan ok %d packed_floats %zu grad_ok %d why %s", (int)plan.ok, plan.packed_floats, (int)plan.grad_ok, plan.why ? plan.why : "-");
        if (k == NS_TRAIN_FWD || k == NS_TRAIN_STEP || k == NS_TRAIN_STEP_BF16)
            dump_adamw(L, in_size, rows, dnp, k == NS_TRAIN_FWD ? 0 : k == NS_TRAIN_STEP ? 1 : 2);
        fputs(g_out.c_str(), stdout);
        printf("== %s | %s G %d Gstride %d nseg %zu LD %d kpad0 %d packed %zu grad %d plan %d | %016llx\n", id, p.ok ? "ok" : "not eligible", p.G,
               p.Gstride, p.ok ? p.seg.size() : (size_t)0, p.LD, p.kpad0, p.packed_floats, (int)p.grad_ok, (int)plan.ok,
               (unsigned long long)fnv1a(g_out));
    }
    return 0;
}
