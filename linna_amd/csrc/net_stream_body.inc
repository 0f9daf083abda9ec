// The body of the whole-network kernels (net_stream.hip: net_stream_kernel, net_stream_train_bf16_kernel,
// net_stream_slice_bf16_kernel, net_stream_grad_bf16_kernel, the EPS / PLAIN / WOUT / DGR instantiations, net_stream_placed_kernel,
// net_stream_trim_kernel), included
// inside each kernel's braces; its template parameters R, MOVE, GRAD, STORE, ROWS, BF, its compile-time flags EPS, PLAIN,
// WOUT and DGR, and its argument NsArgs a are theirs.
    constexpr int NT = NS_NT, NW = NS_NW;
    constexpr int RG = 32;                         // threads per walker row in prologue / reduce / finish
    constexpr bool SM = ROWS < 16;                 // 4x4x1 engine: ROWS / 4 row sets, lane = column
    constexpr int RS = SM ? ROWS / 4 : 1;
    constexpr int NQ = SM ? RS : NT;               // result quads per lane: (row set) or (column tile)
    constexpr int NACC = SM ? 4 * RS : NT;
#ifdef NS_BODY_SLICE_BF16                          // (defined around the include by net_stream_slice_bf16_kernel alone)
    static_assert(BF && !GRAD && STORE == 0 && MOVE == 2, "bf16: the slice evaluation");
#elif defined(NS_BODY_GRAD_BF16)                   // (... by net_stream_grad_bf16_kernel alone)
    static_assert(BF && GRAD && STORE == 2 && MOVE == 0, "bf16: lnP and its gradient in one launch");
#else
    static_assert(!BF || (!GRAD && STORE == 0 && MOVE != 2) || (GRAD && STORE == 3 && MOVE == 0 && ROWS == 4),
                  "bf16: serving, the fused stretch move and the merged training step (4-row engine)");
#endif
    constexpr bool BFT = BF && GRAD && STORE == 3;   // the bf16 training step: one fp32 run (the loss segment) in the stream
    constexpr int AK = BF ? 2 : 1;                 // 16-byte A fragments per lane and step
    constexpr bool K4 = !SM && !BF && (STORE == 0 || (GRAD && STORE == 2));   // 16-row engine, serving and the one-launch gradient: programs may hold SIDE segments
    // (the one-launch gradient with SIDE segments in its forward half was measured SLOWER: 156.4 against 154.2 us at ChtoModelv2(33,33))
    // TRB: a whole training step's network work in ONE launch (linna_net_train_step): gather + transform + forward with the
    // activations kept + chi^2-ratio loss (STORE == 3) as the forward half, the loss finish as the TURNAROUND (loss rows,
    // d loss / d pred to memory AND into LDS as the input of the first backward segment), then the dX chain (STORE == 2's
    // epilogues: gates from the activations this very launch stored, read through the L2) -- one prologue and one launch
    // boundary less than forward + loss and dX chain as two launches, the weight ring never drained in between.
    constexpr bool TRB = GRAD && STORE == 3;
    constexpr bool DXE = STORE == 2 || TRB;        // epilogues of dX segments: gate by the stored activation, store
    constexpr bool G2 = GRAD && STORE == 2;        // lnP + gradient in one launch: nothing of the forward half goes to global memory
    // the gates are sign bits in LDS (NsArgs::nbw).  The merged training launch can gate the same way (LB = G2 || TRB: its
    // launcher fills gbit / mbit), measured SLOWER on its 4-row engine (155.4 against 152.4 us per step at (26,457): the
    // gate loads are not what its run ends wait for, the ballots and bit writes of every forward epilogue are extra) -- off.
    constexpr bool LB = G2;
    constexpr bool LATE_REFILL = true;             // see `step`
    // HAND: the step of the plain serving launch with every instruction placed by hand (net_stream_placed_kernel alone
    // defines NS_BODY_HAND around the include; described at `step`).  The ring, both A fragments and the accumulators then
    // live in FIXED registers -- the asm text names single registers of them -- and are in/out operands of every block.
#ifdef NS_BODY_HAND
    constexpr bool HAND = true;
    static_assert(PLAIN && !BF && ROWS == 16 && R == 6 && NS_NT == 4 && LATE_REFILL, "the hand-placed step: plain fp32 serving, 16 rows, six slots");
#else
    constexpr bool HAND = false;
#endif
    // TRIM: the hand-placed launch without the MFMAs that multiply zero padding (net_stream_trim_kernel alone defines
    // NS_BODY_TRIM next to NS_BODY_HAND; described at the step loop's driver below)
#ifdef NS_BODY_TRIM
    constexpr bool TRIM = true;
    static_assert(HAND, "the trimmed step texts are hand-placed ones");
#else
    constexpr bool TRIM = false;
#endif
    // slot u, tile t: v[128 + 16 u + 4 t ..]; A fragment i: v[224 + 4 i ..]; accumulator t: v[232 + 4 t ..]
#define NS_HAND_RING \
    "+{v[128:131]}"(Bq[0][0]), "+{v[132:135]}"(Bq[0][1]), "+{v[136:139]}"(Bq[0][2]), "+{v[140:143]}"(Bq[0][3]), \
    "+{v[144:147]}"(Bq[1][0]), "+{v[148:151]}"(Bq[1][1]), "+{v[152:155]}"(Bq[1][2]), "+{v[156:159]}"(Bq[1][3]), \
    "+{v[160:163]}"(Bq[2][0]), "+{v[164:167]}"(Bq[2][1]), "+{v[168:171]}"(Bq[2][2]), "+{v[172:175]}"(Bq[2][3]), \
    "+{v[176:179]}"(Bq[3][0]), "+{v[180:183]}"(Bq[3][1]), "+{v[184:187]}"(Bq[3][2]), "+{v[188:191]}"(Bq[3][3]), \
    "+{v[192:195]}"(Bq[4][0]), "+{v[196:199]}"(Bq[4][1]), "+{v[200:203]}"(Bq[4][2]), "+{v[204:207]}"(Bq[4][3]), \
    "+{v[208:211]}"(Bq[5][0]), "+{v[212:215]}"(Bq[5][1]), "+{v[216:219]}"(Bq[5][2]), "+{v[220:223]}"(Bq[5][3])
#define NS_HAND_A "+{v[224:227]}"(Aq[0][0]), "+{v[228:231]}"(Aq[1][0])
#define NS_HAND_ACC "+{v[232:235]}"(acc[0]), "+{v[236:239]}"(acc[1]), "+{v[240:243]}"(acc[2]), "+{v[244:247]}"(acc[3])
    // Non-finite inputs.  Serving and the one-launch gradient poison the row's prior term where x is formed (`zz` in the
    // prologue): lnP = NaN -> -inf whatever the layers make of the row, at no instruction in the layer loop -- their ReLU
    // stays fmaxf, which returns 0 on a NaN.  The forward with stored activations (STORE == 1) has no prior term: its rows
    // arrive transformed (a non-finite x is a NaN there, prior_map_fwd_kernel) and its ReLU keeps the NaN, as torch.relu
    // does, down to the output rows the likelihood launch reads.
    constexpr bool RNAN = STORE == 1;
    auto relu_f = [](float v) { if constexpr (RNAN) return isnan(v) ? v : fmaxf(v, 0.f); else return fmaxf(v, 0.f); };
    static_assert(ROWS == 16 || ROWS == 8 || ROWS == 4, "rows per workgroup");
    static_assert(R % 2 == 0, "the A double buffer alternates with the ring slot parity");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LD = a.LD, ABUF = ROWS * LD;
    // The per-segment tables are indexed at run time.  Through `a` (a by-value argument) such an index makes the compiler
    // keep a private copy of the whole 2.3 KB block whenever it cannot split it -- scratch traffic at every run end, and which
    // instantiation is hit changes with unrelated edits (STORE == 1 on the 16-row engine in round 2, the merged training
    // launch with the refill one slot back in round 3).  Through the kernel-argument segment itself they are scalar loads.
    // (Only in the instantiations where that copy has appeared -- the training ones: the serving ones and the one-launch
    // gradient lose 0.3-0.7 % to the explicit pointer; tests/test_abi.py watches every kernel's scratch size.)
    constexpr bool KA = STORE == 3 || STORE == 1 || GRAD;    // (R4: every GRAD instantiation -- G2 since it holds SIDE code, the MLP gradient since the short-second-pass selects)
    const NsArgs* const ka = KA ? reinterpret_cast<const NsArgs*>((const void*)__builtin_amdgcn_kernarg_segment_ptr()) : &a;
    float* const act = smem;                       // [2][ROWS][LD]
    float* const lbias = smem + 2 * ABUF;          // packed biases of every segment
    unsigned* const lbits = reinterpret_cast<unsigned*>(smem + a.bits_off);   // G2: sign bits [ROWS][nbw]
    const int nbw = a.nbw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * ROWS;
    if constexpr (!PLAIN) {
        if (a.gate && a.gate[0] == 0) return;
    }
    // MOVE == 2 with a row list (the later rounds of linna_slice_half_step): only the trial points of the walkers still
    // active are evaluated -- row r of the launch is trial point mv_C[r] (= j ns + k), mv_step[0] * mv_step_off rows in
    // all, counted on the device; the workgroups behind them leave at once
    int mv_rows = a.B;
    if constexpr (MOVE == 2) {
        if (a.mv_C) {
            mv_rows = a.mv_step[0] * a.mv_step_off;
            if (row0 >= mv_rows) return;
        }
    }
    if constexpr ((STORE == 2 && !GRAD) || TRB) {
        if ((a.p_n > 0 || a.p_step) && blockIdx.x == gridDim.x - 1) {
            // sum_scale_prepare_kernel's arithmetic in its order: 1024 strided partial sums (two per thread here),
            // sixteen wave sums, added in wave order
            float* const part = smem;
            float acc0 = 0.f, acc1 = 0.f;
            for (int i = tid; i < a.p_n; i += 1024) acc0 += a.p_rows[i];
            for (int i = tid + 512; i < a.p_n; i += 1024) acc1 += a.p_rows[i];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { acc0 += __shfl_xor(acc0, o, 64); acc1 += __shfl_xor(acc1, o, 64); }
            if (lane == 0) { part[wave] = acc0; part[8 + wave] = acc1; }
            __syncthreads();
            if (tid == 0 && a.p_out) {
                float t = 0.f;
                for (int w = 0; w < 16; ++w) t += part[w];
                a.p_out[0] = t * a.p_scale;
            }
            if (tid == 64 && a.p_step) {
                const int t = ++a.p_step[0];
                a.p_hyper[2] = (float)(1.0 - pow((double)a.p_b1, (double)t));
                a.p_hyper[3] = (float)sqrt(1.0 - pow((double)a.p_b2, (double)t));
            }
            return;
        }
    }
#ifdef NS_STAMPS
    unsigned long long* const lstamp = reinterpret_cast<unsigned long long*>(lbias + ((a.bias_total + 3) & ~3) + 32 + (a.x0_keep ? 1024 : 0)) + wave * 32;   // (not for GRAD: its masks live there)
    int nstamp = 0;
#define NS_STAMP() do { const unsigned long long t_ = __builtin_readcyclecounter(); \
        if (lane == 0 && nstamp < 32) lstamp[nstamp] = t_; ++nstamp; } while (0)
#define NS_STAMPS_FLUSH() do { if (lane < 32) a.stamps[((size_t)blockIdx.x * NW + wave) * 32 + lane] = lane < nstamp ? lstamp[lane] : 0ull; } while (0)
#else
#define NS_STAMP() do {} while (0)
#define NS_STAMPS_FLUSH() do {} while (0)
#endif
    NS_STAMP();

    // ---- 1. every small load of the kernel, up front, straight-line (no branch on a loaded value)
    const int prt = tid / RG, pc0 = tid % RG;
    const bool prow = prt < ROWS;                   // (ROWS < 16: the thread rows past ROWS only keep the barriers company)
    const int pr = SM ? min(prt, ROWS - 1) : prt;
    int grow = min(row0 + pr, a.B - 1);
    if constexpr (MOVE == 2) {
        if (a.mv_C) grow = a.mv_C[min(row0 + pr, mv_rows - 1)];     // the trial point this row evaluates
    }
    int zsrc = grow;                                // STORE == 3: the row of the resident set this batch row is
    float zden = 1.f;
    if constexpr (STORE == 3) {
        zsrc = a.t_rows ? a.t_rows[grow] : grow;
        zden = a.t_den[zsrc];
    }
    const int kpad0 = a.kpad0, nin = a.nin, nout = a.nout, nseg = a.nseg;
    // PLAIN: the first descriptors of the segment table are touched here, among the argument loads.  A run's request for the
    // next descriptor (plain_request) is the first access to its cache line otherwise, and the miss -- ~500 cycles, measured
    // with the fine stamps -- sits in front of the run's first MFMA with nothing to hide under.
    int seg_warm = 0;
    if constexpr (PLAIN) {
#pragma unroll
        for (int i = 1; i < 8; ++i) seg_warm |= a.seg[i].type | a.seg[i].zext;     // (both 64-byte lines an 8-dword descriptor can span)
    }
    const int nlast = (TRB ? a.nseg_f : nseg) - 2;  // STORE == 3: the network's last layer (the loss segment follows it)
    constexpr int ZPRE = 2;
    float zr[ZPRE], za1[ZPRE], za2[ZPRE], zxm[ZPRE], zxs[ZPRE]; int zfl[ZPRE], zlg[ZPRE];
    const int* const lgp = a.lg ? a.lg : a.is_flat;
    int mv_wk = 0; float mv_factor = 0.f, mv_lnp_old = 0.f, mv_logu = 0.f;
    if constexpr (MOVE == 1) {
        mv_wk = a.mv_S[grow];
        const U4 rb = walker_bits(a.mv_seed, (uint32_t)mv_wk, (uint32_t)(a.mv_step[0] + a.mv_step_off), (uint32_t)a.mv_stream, 0u);
        const float t = (a.mv_a - 1.f) * u01(rb.x) + 1.f;
        const float zf = t * t / a.mv_a;
        const int j = (int)(((uint64_t)rb.y * (uint64_t)a.mv_nc) >> 32);
        const int wc = a.mv_C[j];
        mv_factor = ((float)nin - 1.f) * logf(zf);
        mv_logu = logf(u01(rb.z));
        mv_lnp_old = a.mv_logp[mv_wk];
#pragma unroll
        for (int i = 0; i < ZPRE; ++i) {
            const int c = min(pc0 + i * RG, nin - 1);
            const float cr = a.mv_cc[(size_t)wc * a.mv_ldcc + c], sx = a.mv_coords[(size_t)mv_wk * a.mv_ldc + c];
            zr[i] = cr - (cr - sx) * zf;
        }
    }
    if constexpr (MOVE == 2) {
        // trial points of the ensemble slice sampler, never written to memory: row j*ns + k is
        // coords[S[k]] + w[j*ns + k] * DIR[k]   (what linna_slice_points materialises)
        const int k = grow % a.mv_nc;                                   // mv_nc: ns (walkers per half ensemble)
        const int wk = a.mv_S[k];
        float wgt;
        if (a.sb.logp) {
            // slice_begin_kernel's arithmetic, per row: two distinct complementary walkers, the direction between them, a uniform
            // height under the density, a unit bracket placed uniformly around 0; this row's end of it, jt steps out
            const SliceBegin& b = a.sb;
            const int jt = grow / a.mv_nc;
            const U4 rb = walker_bits(b.seed, (uint32_t)wk, (uint32_t)b.step[0], (uint32_t)b.half, 0u);
            const int ia = (int)(((uint64_t)rb.x * (uint64_t)b.nc) >> 32);
            int ib = (int)(((uint64_t)rb.y * (uint64_t)(b.nc - 1)) >> 32);
            ib += (ib >= ia);
            const int wa = b.C[ia], wb = b.C[ib];
            const float mu = b.mu[0];
            const float l = -u01(rb.w);
            wgt = jt < b.m ? l - (float)jt : l + 1.f + (float)(jt - b.m);
            const bool first = jt == 0 && prow && row0 + pr < a.B;      // the rows that write the walker's state for the later launches
#pragma unroll
            for (int i = 0; i < ZPRE; ++i) {
                const int c = min(pc0 + i * RG, nin - 1);
                const float dir = mu * (b.cc[(size_t)wa * b.ldcc + c] - b.cc[(size_t)wb * b.ldcc + c]);
                zr[i] = a.mv_coords[(size_t)wk * a.mv_ldc + c] + wgt * dir;
                if (first && pc0 + i * RG < nin) b.DIR[(size_t)k * b.ldd + c] = dir;
            }
            if (first && pc0 == 0) {
                b.Z0[k] = b.logp[wk] + logf(u01(rb.z));
                b.L[k] = l; b.R[k] = l + 1.f;
                int J, K;
                slice_budget(b.seed, (uint32_t)wk, (uint32_t)b.step[0], (uint32_t)b.half, b.maxsteps, J, K);
                b.flags[3 * k] = J; b.flags[3 * k + 1] = K; b.flags[3 * k + 2] = 1;
            }
            if (blockIdx.x == 0 && tid == 0) {
                for (int i = 0; i < b.nslots; ++i) {       // [4 + nslots + i]: the same counts summed over the calls so far (usage statistics)
                    b.counters[4 + b.nslots + i] += b.counters[4 + i];
                    b.counters[4 + i] = 0;
                }
                b.counters[4 + 2 * b.nslots] += 1;         // calls
                if (b.zero_totals) { b.counters[0] = 0; b.counters[1] = 0; }
            }
        } else {
        if (a.sl_Zt) {
            // lanes 0 .. 2 m - 1 of the row's 32 hold "lnP at bracket end j exceeds Z0"; the count of leading ones per side is
            // the number of steps out.  Lane i < nt holds the uniform of trial i; the row walks the trials up to its own.
            const int ns_ = a.mv_nc, m = a.sl_m, jt = grow / ns_;
            const float z0 = a.sl_Z0[k];
            const float zend = a.sl_Zt[(size_t)min(pc0, 2 * m - 1) * ns_ + k];
            const unsigned long long bal = __ballot(pc0 < 2 * m && zend > z0);
            const unsigned bits = (unsigned)(bal >> (lane & 32));
            const unsigned lm = bits & ((1u << m) - 1u), rm = (bits >> m) & ((1u << m) - 1u);
            // (never more steps than the budget of that side has left: slice_side_steps in common.h)
            const int nl = min(__builtin_ctz(~lm), a.sl_flags[3 * k]), nr = min(__builtin_ctz(~rm), a.sl_flags[3 * k + 1]);
            float l = a.sl_L[k], r = a.sl_R[k];
            for (int j = 0; j < m; ++j) {                               // (one unit at a time: the rounding of slice_expand_multi_kernel)
                if (j < nl) l -= 1.f;
                if (j < nr) r += 1.f;
            }
            const U4 tb = walker_bits(a.sl_seed, (uint32_t)wk, (uint32_t)a.sl_step[0], (uint32_t)a.sl_stream, (uint32_t)(pc0 + 1));
            const int myu = __float_as_int(u01(tb.x));
            wgt = 0.f;
            for (int jj = 0; jj < a.sl_nt; ++jj) {
                const int ulo = __builtin_amdgcn_readlane(myu, jj), uhi = __builtin_amdgcn_readlane(myu, 32 + jj);
                const float u = __int_as_float((lane & 32) ? uhi : ulo);
                const float w = l + u * (r - l);
                if (jj == jt) wgt = w;
                if (jj < jt) { if (w < 0.f) l = w; else r = w; }
            }
        } else {
            wgt = a.mv_cc[grow];                                        // mv_cc: w[nrep * ns]
        }
#pragma unroll
        for (int i = 0; i < ZPRE; ++i) {
            const int c = min(pc0 + i * RG, nin - 1);
            zr[i] = a.mv_coords[(size_t)wk * a.mv_ldc + c] + wgt * a.Z[(size_t)k * a.ldz + c];   // Z: DIR[ns][ldz]
        }
        }
    }
#pragma unroll
    for (int i = 0; i < ZPRE; ++i) {
        const int c = min(pc0 + i * RG, nin - 1);
        if constexpr (MOVE == 0) zr[i] = a.Z[(size_t)(STORE == 3 ? zsrc : grow) * a.ldz + c];
        zfl[i] = a.is_flat[c]; za1[i] = a.a1[c]; za2[i] = a.a2[c];
        zlg[i] = lgp[c]; zxm[i] = a.xmean[c]; zxs[i] = a.xstd[c];
    }
    const int nb4 = (a.bias_total + 3) >> 2;       // packed biases, 16 bytes per thread and round
    const f32x4* const bsrc = reinterpret_cast<const f32x4*>(a.packed + (size_t)NW * a.Gstride * NT * 256);
    constexpr int BMAX = 3;                        // 3 x 512 x 4 floats >= every eligible network's biases
    f32x4 breg[BMAX];
#pragma unroll
    for (int i = 0; i < BMAX; ++i) {
        const int j = tid + i * 64 * NW;
        breg[i] = bsrc[min(j, nb4 - 1)];
    }
    constexpr int FIN = 2;
    const float* const csp = a.cscale ? a.cscale : a.xmean;   // always a readable pointer
    const float* const ctp = a.cshift ? a.cshift : a.xmean;
    const float* const wtp = a.w ? a.w : a.xmean;
    float fcs[FIN], fct[FIN], fw[FIN], fgs[FIN];
#pragma unroll
    for (int i = 0; i < FIN; ++i) {
        const int cc = min(pc0 + i * RG, nout - 1);
        if constexpr (DGR) {                       // the output map and the covariance are in the stream: nothing to load
            fgs[i] = 0.f; fcs[i] = 1.f; fct[i] = 0.f; fw[i] = 0.f;
            continue;
        }
        if constexpr (GRAD && !TRB) fgs[i] = a.gscale[cc]; else fgs[i] = 0.f;
        if constexpr (PLAIN) {                     // (the launcher hands over all three)
            fcs[i] = a.cscale[cc]; fct[i] = a.cshift[cc]; fw[i] = a.w[cc];
        } else {
        const int c1 = a.cscale ? cc : 0, c2 = a.cshift ? cc : 0, c3 = a.w ? cc : 0;
        const float cs = csp[c1], ct = ctp[c2], ww = wtp[c3];
        fcs[i] = a.cscale ? cs : 1.f; fct[i] = a.cshift ? ct : 0.f; fw[i] = a.w ? ww : 0.f;
        }
    }

    // ---- 2. weight stream: wave-uniform base + 32-bit per-lane offset + immediate
    const char* const wbase = reinterpret_cast<const char*>(a.packed) + (size_t)wave * a.Gstride * NS_STEP_B;
    const unsigned wlast = (unsigned)(a.G - 1) * NS_STEP_B;
    unsigned woff = 0;
    const unsigned voff = 16u * (unsigned)lane;
    f32x4 Bq[R][NT];
    auto wload = [&](int t) { return *reinterpret_cast<const f32x4*>(wbase + (size_t)(voff + woff) + t * 1024); };
    auto wadvance = [&]() { woff = min(woff + NS_STEP_B, wlast); };   // past the end: reload the last step (never used)
    constexpr int PRE = NS_PRE < R ? NS_PRE : R;
    auto prefetch = [&](auto Uc) {
        constexpr int U = decltype(Uc)::value;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            Bq[U][t] = wload(t);
            __builtin_amdgcn_sched_barrier(0);     // keep the issue order: the loop's counted vmcnt depends on it
        }
        wadvance();
    };
#define NS_PF(U, LO, HI) if constexpr (U >= LO && U < HI) prefetch(std::integral_constant<int, U>{});
#define NS_PF_ALL(LO, HI) NS_PF(0, LO, HI) NS_PF(1, LO, HI) NS_PF(2, LO, HI) NS_PF(3, LO, HI) NS_PF(4, LO, HI) NS_PF(5, LO, HI) \
    NS_PF(6, LO, HI) NS_PF(7, LO, HI)
    NS_PF_ALL(0, PRE)
#ifdef NS_STAMPS_FINE
    NS_STAMP();                                    // every small load and the first weight slots requested
#endif

    // ---- 3. network input x = X_transform(Transform(z)) into buffer 0, zero padded to kpad0; biases to LDS
    float zz = 0.f;
    float theta[ZPRE];
#pragma unroll
    for (int i = 0; i < ZPRE; ++i) {
        const int c = pc0 + i * RG;
        const bool in = c < nin;
        const float z = in ? zr[i] : 0.f;
        zz += z * z;
        float th = ns_prior_theta(z, zfl[i], za1[i], za2[i]);
        float lt = th;
        if (!TRIM || a.lg) {                        // (TRIM: a launch without a log10 index computes none -- a wave-uniform test)
            lt = log10f(th);
            asm volatile("" : "+v"(lt));
        }
        theta[i] = th;
        const float t = (a.lg && zlg[i]) ? lt : th;
        float x = in ? (t - zxm[i]) / zxs[i] : 0.f;
        zz += 0.f * x;                              // a non-finite input (log10 of theta <= 0) poisons the row's prior term: lnP = -inf
        if constexpr ((STORE == 1 || STORE == 2) && !GRAD) x = z;   // rows arrive transformed
        if constexpr (STORE == 3) {                 // X_transform of a gathered row (util.py:483-497), as linna_gather_xform
            float lz = log10f(z);
            asm volatile("" : "+v"(lz));
            const float tz = (a.lg && zlg[i]) ? lz : z;
            x = in ? (tz - zxm[i]) / zxs[i] : 0.f;
            if (prow && row0 + pr < a.B && c < a.t_ldxb)
                asm volatile("global_store_dword %0, %1, off" :: "v"(a.t_xb + (size_t)(row0 + pr) * a.t_ldxb + c), "v"(x) : "memory");
        }
        if constexpr (BF) {                         // x_hi at c, x_lo at nin + c, zeros from 2 nin (net_program.hip, ns_lower: [W | W])
            if (prow) {
                if (in) { const float hi = (float)(__bf16)x; act[pr * LD + c] = hi; act[pr * LD + nin + c] = x - hi; }
                else if (c >= 2 * nin && c < kpad0) act[pr * LD + c] = 0.f;
            }
        } else {
            if (c < kpad0 && prow) act[pr * LD + c] = x;
        }
    }
#ifdef NS_STAMPS_FINE
    NS_STAMP();                                    // first 64 input columns transformed and in LDS
#endif
    // inputs wider than ZPRE*RG = 64 columns (none of the reference's models; <= 256 supported) and the zero
    // pad of a SPLIT first segment: plain loop, loads waited in place
    if constexpr ((STORE == 1 || STORE == 2) && !GRAD) {
        // rows arrive transformed (the dX chain's input is d loss / d pred, 457 or 1000 columns wide): every thread of the
        // workgroup copies, four independent loads in flight each -- the per-row loop below waits for every load in place
        const int wcols = kpad0 - ZPRE * RG;
        if (wcols > 0) {
            constexpr int CP = 4;
            for (int base = 0; base < ROWS * wcols; base += CP * 64 * NW) {
                float v[CP];
#pragma unroll
                for (int u = 0; u < CP; ++u) {
                    const int idx = min(base + u * 64 * NW + tid, ROWS * wcols - 1);
                    const int r = idx / wcols, c = ZPRE * RG + idx % wcols;
                    v[u] = a.Z[(size_t)min(row0 + r, a.B - 1) * a.ldz + min(c, nin - 1)];
                }
#pragma unroll
                for (int u = 0; u < CP; ++u) {
                    const int idx = base + u * 64 * NW + tid;
                    if (idx < ROWS * wcols) {
                        const int r = idx / wcols, c = ZPRE * RG + idx % wcols;
                        act[r * LD + c] = c < nin ? v[u] : 0.f;
                    }
                }
            }
        }
    } else
#pragma unroll 1
    for (int c = pc0 + ZPRE * RG; c < kpad0; c += RG) {
        float x = 0.f;
        if (c < nin) {
            const float z = a.Z[(size_t)grow * a.ldz + c];
            zz += z * z;
            const float th = ns_prior_theta(z, a.is_flat[c], a.a1[c], a.a2[c]);
            const float t = (a.lg && a.lg[c]) ? log10f(th) : th;
            x = (t - a.xmean[c]) / a.xstd[c];
            zz += 0.f * x;
            if constexpr ((STORE == 1 || STORE == 2) && !GRAD) x = z;
            if constexpr (STORE == 3) {
                const float zz3 = a.Z[(size_t)zsrc * a.ldz + c];
                x = (((a.lg && a.lg[c]) ? log10f(zz3) : zz3) - a.xmean[c]) / a.xstd[c];
            }
        }
        if constexpr (STORE == 3) {
            if (prow && row0 + pr < a.B && c < a.t_ldxb)
                asm volatile("global_store_dword %0, %1, off" :: "v"(a.t_xb + (size_t)(row0 + pr) * a.t_ldxb + c), "v"(x) : "memory");
        }
        if constexpr (BF) {
            if (prow) {
                if (c < nin) { const float hi = (float)(__bf16)x; act[pr * LD + c] = hi; act[pr * LD + nin + c] = x - hi; }
                else if (c >= 2 * nin) act[pr * LD + c] = 0.f;
            }
        } else {
            if (prow) act[pr * LD + c] = x;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#ifdef NS_STAMPS_FINE
    NS_STAMP();                                    // the rest of the input in LDS
#endif
    NS_PF_ALL(PRE, (LATE_REFILL ? R - 1 : R))
#undef NS_PF_ALL
#undef NS_PF
#pragma unroll
    for (int o = RG / 2; o >= 1; o >>= 1) zz += __shfl_xor(zz, o, 64);
#pragma unroll
    for (int i = 0; i < BMAX; ++i) {
        const int j = tid + i * 64 * NW;
        if (j < nb4) reinterpret_cast<f32x4*>(lbias)[j] = breg[i];
    }
    int* const lsrc = reinterpret_cast<int*>(lbias + ((a.bias_total + 3) & ~3));      // STORE == 3: [ROWS] set rows, [ROWS] den
    float* const lden = reinterpret_cast<float*>(lsrc + 16);
    if constexpr (STORE == 3) {
        if (prow && pc0 == 0) { lsrc[pr] = zsrc; lden[pr] = zden; }
    }
    float* const lx0 = lden + 16;                  // [ROWS][64]: the input rows, for a later input-skip segment
    if constexpr (!PLAIN) {
    if (a.x0_keep && prow) {
#pragma unroll
        for (int i = 0; i < ZPRE; ++i) {
            const int c = pc0 + i * RG;
            if constexpr (BF) lx0[pr * 64 + c] = c < nin ? act[pr * LD + c] + act[pr * LD + nin + c] : 0.f;   // x_hi + x_lo = x exactly
            else lx0[pr * 64 + c] = (c < kpad0) ? act[pr * LD + c] : 0.f;
        }
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                  // raw: __syncthreads() would drain the weight stream
    asm volatile("" ::: "memory");
    NS_STAMP();

    if constexpr (HAND) {
        // From here on the compiler sees no vector-memory instruction and counts none: every later wait for the ring is
        // written out in the step's text.  The prologue's own loads (compiled C++) are waited for HERE, once, outside the
        // loop -- as operands of the first step they would put a compiler-made vmcnt(0) at the loop's head.  They were
        // requested in front of the bias copy and the barrier, a thousand cycles and more ago.
#pragma unroll
        for (int t = 0; t < NT; ++t) Bq[R - 1][t] = f32x4{0.f, 0.f, 0.f, 0.f};      // (the slot the first step refills)
        asm volatile("" : NS_HAND_RING :: "memory");
    }
    // ---- 4. the step loop
    const uint32_t act_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)act;
    f32x4 acc[NACC];
    f32x4 Aq[2][AK];
    // 4x4x1 engine: block b = lane >> 2 of the A read holds row set b & 3 (rows wrap below ROWS: never selected), k chunk b >> 2
    const int sm_arow = (4 * ((lane >> 2) & 3) + (lane & 3)) % ROWS, sm_achunk = lane >> 4;
    int si = 0, pass = 0, P = 0, kleft;
    int s_type, s_steps, s_passes, s_bias, s_dst, s_relu, s_kslice, s_zext, s_ncgl, s_mstore = 0, s_mapply = 0, s_x0col = 0, s_x0n = 0, s_kcl = 0;
    // TRIM: the segment's output width N and whether the last step of its runs holds one live k slice (both folded into
    // NsSeg::type by the launcher), the choice of step text for the run in flight (s_trim: bit 0 every step T3, bit 1 the last
    // S1), and the operands of the step's text: the ring slot the next step consumes, the ring of texts, the steps to run
    int s_N = 0, s_sl1 = 0, s_trim = 0, s_sel = 0, s_tx = 0, s_n = 0;
    unsigned* const lmask = reinterpret_cast<unsigned*>(lbias + ((a.bias_total + 3) & ~3));   // GRAD: [slot][512 lanes]
    float lnp_grad = 0.f;                          // GRAD: lnP, stored at the very end (no store next to the weight loads)
    float* s_gout = nullptr; int s_gld = 0, s_gn = 0;   // STORE: global destination of the current segment's output
    const float* s_gmask = nullptr; int s_gmld = 0;     // STORE == 2: forward activation gating it
    int s_gbit = -1, s_mbit = -1;                       // LB: bit column of the signs this segment writes / is gated by
    auto gstore = [&](float* p, float v) { asm volatile("global_store_dword %0, %1, off" :: "v"(p), "v"(v) : "memory"); };
    uint32_t ap;
    // BFT: the run of segment nseg_f - 1 (the loss segment) is fp32, 16 k per step: one fragment, 64 bytes per step
    auto a_read = [&](f32x4* dst) {
        if constexpr (HAND) {                      // straight into the fragment's fixed registers: no copy of a value still in flight
            if (dst == Aq[0]) asm volatile("ds_read_b128 %0, %1" : "={v[224:227]}"(Aq[0][0]) : "v"(ap) : "memory");
            else asm volatile("ds_read_b128 %0, %1" : "={v[228:231]}"(Aq[1][0]) : "v"(ap) : "memory");
        } else
        asm volatile("ds_read_b128 %0, %1" : "=v"(dst[0]) : "v"(ap) : "memory");
        if constexpr (BF) asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(dst[1]) : "v"(ap) : "memory");
        if constexpr (BFT) ap += si == a.nseg_f - 1 ? 64 : 64 * AK;
        else ap += 64 * AK;
    };
    // (kernel-argument arrays are indexed through readfirstlane: one instantiation -- STORE == 1 on the 16-row engine --
    // could not prove the segment index uniform and copied the whole 2 KB argument block to scratch)
    auto load_seg = [&]() {
        const NsSeg S = ka->seg[__builtin_amdgcn_readfirstlane(si)];
        s_type = S.type; kleft = s_steps = S.steps; s_passes = S.passes; s_bias = S.bias_off;
        s_dst = S.dst_col; s_relu = S.relu; s_kslice = S.kslice; s_zext = S.zext; s_ncgl = S.ncg_log2; s_x0col = S.x0_col; s_x0n = S.x0_n;
        if constexpr (GRAD) { s_mstore = S.mask_store; s_mapply = S.mask_apply; }
        if constexpr (STORE) { const int j = __builtin_amdgcn_readfirstlane(si); s_gout = ka->gout[j]; s_gld = ka->gld[j]; s_gn = ka->gn[j]; }
        if constexpr (DXE) { const int j = __builtin_amdgcn_readfirstlane(si); s_gmask = ka->gmask[j]; s_gmld = ka->gmld[j]; }
        if constexpr (LB) { const int j = __builtin_amdgcn_readfirstlane(si); s_gbit = ka->gbit[j]; s_mbit = ka->mbit[j]; }
    };
    // PLAIN: the NEXT segment's descriptor sits in scalar registers from the start of the current run (requested behind the
    // run's first A read; the wait of the next step for that fragment covers it), so no run end waits for a scalar load.
    // Eight fields: a plain program reads nothing else, and the launcher folds ncg_log2 into the upper bits of `type`.
    NsSeg nxp;
    auto plain_request = [&]() { nxp = ka->seg[__builtin_amdgcn_readfirstlane(min(si + 1, nseg - 1))]; };
    auto plain_take = [&](const NsSeg& X) {
        s_type = X.type & 255; kleft = s_steps = X.steps; s_passes = X.passes; s_bias = X.bias_off;
        if constexpr (TRIM) { s_ncgl = (X.type >> 8) & 15; s_N = (X.type >> 12) & 4095; s_sl1 = ((X.type >> 24) & 3) == 0 ? 2 : 0; }
        else s_ncgl = X.type >> 8;
        s_dst = X.dst_col; s_relu = X.relu; s_kslice = X.kslice; s_zext = X.zext;
    };
    auto begin_run = [&]() {                       // accumulators and A pointer of run (si, pass)
        const int arow = SM ? sm_arow : li, ak = AK * (SM ? 4 * sm_achunk : 4 * kq);
#pragma unroll
        for (int t = 0; t < NACC; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (s_type == NS_WIDE) {
            // the wave's 64-column block of this run: 8 pass + wave -- or, balanced triangular factor (zext < 0), w then 15 - w
            // (PLAIN: a plain program has neither the triangular factor nor a short second pass)
            const int blk = !PLAIN && s_zext < 0 ? (pass ? 15 - wave : wave) : 8 * pass + wave;
            if constexpr (SM) {
                const float b = lbias[s_bias + 64 * blk + lane];
#pragma unroll
                for (int r = 0; r < RS; ++r) acc[4 * r] = f32x4{b, b, b, b};
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float b = lbias[s_bias + 16 * (4 * blk + t) + li];
                    acc[t] = f32x4{b, b, b, b};
                }
            }
            if (!PLAIN && s_zext < 0) kleft = s_steps - 4 * blk;             // its rows start at 64 blk
            ap = act_lds + 4u * (uint32_t)(P * ABUF + arow * LD + ak + (PLAIN ? 0 : s_zext < 0 ? 64 * blk : (pass ? s_kslice : 0)));   // (kslice: 0 but for a short second pass)
        } else {
            ap = act_lds + 4u * (uint32_t)(P * ABUF + arow * LD + ak + (wave >> s_ncgl) * s_kslice);
        }
        if constexpr (BFT) {
            if (si == a.nseg_f - 1) ap -= 4u * (uint32_t)(ak / 2);     // the fp32 loss run: 4 k per lane and step, not 8
        }
        // HAND: the run's first MFMAs sit in asm text, where the compiler's hazard recogniser pads nothing: the wait states
        // between the vector writes of the accumulators above and an MFMA that reads them are spent here
        if constexpr (HAND) asm volatile("s_nop 3" : NS_HAND_ACC);
        // TRIM: the wave's 64-column block of this run starts at column c0 of N; with 33 .. 48 real columns in it the fourth
        // 16-column tile is padding (tlive == 3)
        if constexpr (TRIM) {
            const int c0 = 64 * (s_type == NS_WIDE ? 8 * pass + wave : wave & ((1 << s_ncgl) - 1));
            s_trim = __builtin_amdgcn_readfirstlane(s_sl1 | (s_N - c0 > 32 && s_N - c0 <= 48 ? 1 : 0));
        }
    };
    auto lds_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    if constexpr (PLAIN) {
        asm volatile("" :: "s"(seg_warm));          // (the touches above are loads nobody else waits for)
        plain_take(ka->seg[0]); begin_run(); a_read(Aq[0]); plain_request();
    }
    else {
    load_seg();
    begin_run();
    a_read(Aq[0]);
    }

    // TX: 0 the whole step -- its text, the count and the run end.  TRIM's loop takes the parts one at a time: 5 the text of
    // a whole run from slot s_sel (s_n steps, full or T3 by s_tx) or of one S1 step (below), 4 the run end alone (the slot is
    // a run-time value then, not U).
    auto step = [&](auto Uc, auto Refill, auto Txc) {
        constexpr int U = decltype(Uc)::value;
        constexpr bool refill = decltype(Refill)::value;
        constexpr int TX = decltype(Txc)::value;
        static_assert(TX == 0 || (TRIM && refill), "parts of a step: the trimmed launch, whose steps always refill");
        if constexpr (TX != 4) {
        // the refill of this step goes to the slot the PREVIOUS step consumed: a load whose target the MFMAs just issued
        // still read waits for them at issue (measured: the same loads one slot back, 1.2-1.4 % off every launch; R - 1
        // steps are in flight instead of R).  Not in the merged training launch: its register allocation does not survive
        // the longer slot lifetimes (2.3 KB of scratch per lane, +40 % on the step).
        constexpr int RU = LATE_REFILL ? (U + R - 1) % R : U;
        if constexpr (HAND) {
            // The same step -- the same sixteen MFMAs on the same fragments in the same order, the same four loads from the
            // same addresses into the slot the previous step consumed, the same A read -- as ONE block of text, at most one
            // vector-issue filler per MFMA gap: the A read behind the first MFMA, one refill load behind the third, fifth,
            // seventh and ninth, the A pointer's add behind the eleventh, and each counted wait directly in front of the first
            // MFMA that reads its tile.  An MFMA holds the SIMD's vector issue for 8 of its 32 cycles; the compiled step of the
            // plain instantiation issues the four loads as one block behind its twelfth MFMA, an s_nop 7 in front of them, and
            // pads in front of loads spread from C++ (NOTES 3.1b R3, "Hand-placed step").  The wave's stream address is an SGPR pair (base + the step's offset, advanced on the scalar
            // unit between the blocks), the lane's 16 bytes a constant VGPR, the tile the immediate: no vector add for it.
            // vmcnt: 5 slots = 20 loads are in flight at the start of every step, the oldest four this step's (the
            // prologue requests R - 1 slots, every step of the main loop refills one -- past the end the last one again --
            // and tail step U, which refills nothing, starts with 20 - 4 U).  Tile t with j refills of this step issued:
            // all but the youngest 19 - t + j.
            // Hazards the text owns: the first load reads the SGPR pair seven instructions into the block (five wait states
            // after a scalar write); the accumulators' vector writes and reads are kept away from the MFMAs by the s_nop of
            // begin_run and of the run end below.
            constexpr int BU = 128 + 16 * U, BR = 128 + 16 * RU, AC = 224 + 4 * (U & 1), AN = 224 + 4 * ((U + 1) & 1);
            constexpr int TW = refill ? 0 : 4 * U;       // loads a tail step does not find in flight
#define NS_XM(AC, BU, t, s) "v_mfma_f32_16x16x4_f32 v[232+4*" #t ":235+4*" #t "], v[" #AC "+" #s "], v[" #BU "+4*" #t "+" #s "], v[232+4*" #t ":235+4*" #t "]\n\t"
#define NS_XLS(SB, RU, t, off) "global_load_dwordx4 v[" #RU "+4*" #t ":" #RU "+4*" #t "+3], %[vo], " #SB " offset:" #off "\n\t"
#define NS_HM(t, s) NS_XM(%[ac], %[bu], t, s)
#define NS_HL(t, off) NS_XLS(%[sb], %[ru], t, off)
#define NS_XL(RU, t, off) NS_XLS(vcc, RU, t, off)
#define NS_HAND_TEXT(HEAD, L0, L1, L2, L3) HEAD \
            "s_waitcnt lgkmcnt(0)\n\t" \
            "s_waitcnt vmcnt(%[w0])\n\t" \
            NS_HM(0, 0) "ds_read_b128 v[%[an]:%[an]+3], %[ap]\n\t" \
            "s_waitcnt vmcnt(%[w1])\n\t" \
            NS_HM(1, 0) \
            NS_HM(0, 1) L0 \
            NS_HM(1, 1) \
            NS_HM(0, 2) L1 \
            NS_HM(1, 2) \
            NS_HM(0, 3) L2 \
            NS_HM(1, 3) \
            "s_waitcnt vmcnt(%[w2])\n\t" \
            NS_HM(2, 0) L3 \
            "s_waitcnt vmcnt(%[w3])\n\t" \
            NS_HM(3, 0) \
            NS_HM(2, 1) "v_add_u32 %[ap], 64, %[ap]\n\t" \
            NS_HM(3, 1) NS_HM(2, 2) NS_HM(3, 2) NS_HM(2, 3) NS_HM(3, 3)
            // TRIM, two shorter texts of the same step: same registers, same four refill loads, same A read and pointer add,
            // the counted wait in front of the first MFMA that reads a tile.
            // T3: the wave's fourth column tile is padding nobody reads -- its four MFMAs are left out (its load is not: the
            // count of loads in flight stays what every later wait assumes).
            // S1: the last step of a run whose K ends one k into it -- the slices s = 1, 2, 3 of every tile are the zero fill
            // times the zero pad, added to accumulators slice 0 has already pushed through +0: left out.  With no refill
            // issued in front of tile 2's MFMA and one in front of tile 3's, their waits are 19 - t + j = 17 and 17; the first
            // load sits nine instructions into the text.
            // TRIM's steps (TX == 5) are ONE block: a run of s_n steps from slot s_sel -- the six texts in a ring, full (s_tx
            // == 0: the hidden layers) or T3 (s_tx == 1), the run's count and its test on the scalar unit behind each, which is
            // what the compiled loop spends on --kleft == 0 -- or, s_n == 0, the single S1 step of slot s_sel, all chosen by
            // scalar compares in front.  The compiler sees one statement with the ring, the fragments and the accumulators as
            // its operands, as in every other step, and a loop of that statement and ONE run end.  (As eighteen statements in
            // a switch beside compiled six-step groups the register allocation did not hold: 250 B of scratch.)  The stream
            // address is advanced in the text too, on the scalar unit behind the step's last load: the pair is VCC (the next
            // step's first load reads it seven instructions and more into its text).
#define NS_XHEAD(AC, AN, BU) \
            "s_waitcnt lgkmcnt(0)\n\t" \
            "s_waitcnt vmcnt(19)\n\t" \
            NS_XM(AC, BU, 0, 0) "ds_read_b128 v[" #AN ":" #AN "+3], %[ap]\n\t" \
            "s_waitcnt vmcnt(18)\n\t" \
            NS_XM(AC, BU, 1, 0)
#define NS_XHALF(AC, BU, RU) \
            NS_XM(AC, BU, 0, 1) NS_XL(RU, 0, 0) \
            NS_XM(AC, BU, 1, 1) \
            NS_XM(AC, BU, 0, 2) NS_XL(RU, 1, 1024) \
            NS_XM(AC, BU, 1, 2) \
            NS_XM(AC, BU, 0, 3) NS_XL(RU, 2, 2048) \
            NS_XM(AC, BU, 1, 3) \
            "s_waitcnt vmcnt(20)\n\t" \
            NS_XM(AC, BU, 2, 0) NS_XL(RU, 3, 3072) NS_XADV
#define NS_XADV \
            "s_add_u32 %[wo], %[wo], 0x1000\n\t" "s_min_u32 %[wo], %[wo], %[wl]\n\t" \
            "s_add_u32 vcc_lo, %[wbl], %[wo]\n\t" "s_addc_u32 vcc_hi, %[wbh], 0\n\t"
#define NS_XADD "v_add_u32 %[ap], 64, %[ap]\n\t"
#define NS_XFULL(AC, AN, BU, RU) NS_XHEAD(AC, AN, BU) NS_XHALF(AC, BU, RU) \
            "s_waitcnt vmcnt(20)\n\t" \
            NS_XM(AC, BU, 3, 0) \
            NS_XM(AC, BU, 2, 1) NS_XADD \
            NS_XM(AC, BU, 3, 1) NS_XM(AC, BU, 2, 2) NS_XM(AC, BU, 3, 2) NS_XM(AC, BU, 2, 3) NS_XM(AC, BU, 3, 3)
#define NS_XT3(AC, AN, BU, RU) NS_XHEAD(AC, AN, BU) NS_XHALF(AC, BU, RU) \
            NS_XM(AC, BU, 2, 1) NS_XADD \
            NS_XM(AC, BU, 2, 2) NS_XM(AC, BU, 2, 3)
#define NS_XS1(AC, AN, BU, RU) NS_XHEAD(AC, AN, BU) \
            "s_waitcnt vmcnt(17)\n\t" \
            NS_XM(AC, BU, 2, 0) NS_XL(RU, 0, 0) \
            "s_waitcnt vmcnt(17)\n\t" \
            NS_XM(AC, BU, 3, 0) NS_XL(RU, 1, 1024) NS_XL(RU, 2, 2048) NS_XL(RU, 3, 3072) NS_XADV \
            NS_XADD
            // slot U: fragment read AC, fragment requested AN, ring slot consumed BU, ring slot refilled RU (the one before)
#define NS_XRING(L, TEXT) \
            "s_cmp_eq_u32 %[sel], 1\n\t" "s_cbranch_scc1 " #L "1f\n\t" "s_cmp_eq_u32 %[sel], 2\n\t" "s_cbranch_scc1 " #L "2f\n\t" \
            "s_cmp_eq_u32 %[sel], 3\n\t" "s_cbranch_scc1 " #L "3f\n\t" "s_cmp_eq_u32 %[sel], 4\n\t" "s_cbranch_scc1 " #L "4f\n\t" \
            "s_cmp_eq_u32 %[sel], 5\n\t" "s_cbranch_scc1 " #L "5f\n\t" \
            ".p2align 3\n" \
            #L "0:\n\t" TEXT(224, 228, 128, 208) NS_XCNT #L "1:\n\t" TEXT(228, 224, 144, 128) NS_XCNT \
            #L "2:\n\t" TEXT(224, 228, 160, 144) NS_XCNT #L "3:\n\t" TEXT(228, 224, 176, 160) NS_XCNT \
            #L "4:\n\t" TEXT(224, 228, 192, 176) NS_XCNT #L "5:\n\t" TEXT(228, 224, 208, 192) NS_XCNT \
            "s_branch " #L "0b\n"
#define NS_XCNT "s_add_u32 %[n], %[n], -1\n\t" "s_cmp_eq_u32 %[n], 0\n\t" "s_cbranch_scc1 99f\n"
#define NS_XONE(U, AC, AN, BU, RU) \
            "s_cmp_lg_u32 %[sel], " #U "\n\t" "s_cbranch_scc1 1" #U "f\n\t" NS_XS1(AC, AN, BU, RU) "s_branch 99f\n" "1" #U ":\n\t"
            if constexpr (TX == 5) {
                static_assert(NS_STEP_B == 0x1000, "the stream advance in the text");
                const unsigned wbl = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)wbase);
                const unsigned wbh = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)wbase >> 32));
                asm volatile("s_add_u32 vcc_lo, %[wbl], %[wo]\n\t" "s_addc_u32 vcc_hi, %[wbh], 0\n\t"
                             "s_cmp_eq_u32 %[n], 0\n\t" "s_cbranch_scc1 60f\n\t"
                             "s_cmp_lg_u32 %[tx], 0\n\t" "s_cbranch_scc1 58f\n\t"
                             NS_XRING(4, NS_XFULL)
                             "58:\n\t" NS_XRING(5, NS_XT3)
                             "60:\n\t"
                             NS_XONE(0, 224, 228, 128, 208) NS_XONE(1, 228, 224, 144, 128) NS_XONE(2, 224, 228, 160, 144)
                             NS_XONE(3, 228, 224, 176, 160) NS_XONE(4, 224, 228, 192, 176) NS_XONE(5, 228, 224, 208, 192) "99:\n\t"
                             : NS_HAND_RING, NS_HAND_A, NS_HAND_ACC, [ap] "+v"(ap), [wo] "+s"(woff), [n] "+s"(s_n)
                             : [vo] "v"(voff), [wbl] "s"(wbl), [wbh] "s"(wbh), [wl] "s"(wlast),
                               [sel] "s"(__builtin_amdgcn_readfirstlane(s_sel)), [tx] "s"(__builtin_amdgcn_readfirstlane(s_tx)) : "memory", "scc", "vcc");
            } else
            if constexpr (refill) {
                const char* const sb = wbase + woff;
                // the loop's head is 8-byte aligned: hand-written streams are sensitive to a 4-byte phase of their code
                // (-DNS_HAND_PHASE4, a diagnostic build: the same stream 4 bytes on -- NOTES has both)
#ifdef NS_HAND_PHASE4
#define NS_HAND_HEAD ".p2align 3\n\ts_nop 0\n\t"
#else
#define NS_HAND_HEAD ".p2align 3\n\t"
#endif
                if constexpr (U == 0)
                    asm volatile(NS_HAND_TEXT(NS_HAND_HEAD, NS_HL(0, 0), NS_HL(1, 1024), NS_HL(2, 2048), NS_HL(3, 3072))
                                 : NS_HAND_RING, NS_HAND_A, NS_HAND_ACC, [ap] "+v"(ap)
                                 : [vo] "v"(voff), [sb] "s"(sb), [bu] "n"(BU), [ru] "n"(BR), [ac] "n"(AC), [an] "n"(AN),
                                   [w0] "n"(19), [w1] "n"(18), [w2] "n"(20), [w3] "n"(20) : "memory");
                else
                    asm volatile(NS_HAND_TEXT("", NS_HL(0, 0), NS_HL(1, 1024), NS_HL(2, 2048), NS_HL(3, 3072))
                                 : NS_HAND_RING, NS_HAND_A, NS_HAND_ACC, [ap] "+v"(ap)
                                 : [vo] "v"(voff), [sb] "s"(sb), [bu] "n"(BU), [ru] "n"(BR), [ac] "n"(AC), [an] "n"(AN),
                                   [w0] "n"(19), [w1] "n"(18), [w2] "n"(20), [w3] "n"(20) : "memory");
                wadvance();
            } else {
                asm volatile(NS_HAND_TEXT("", "", "", "", "")
                             : NS_HAND_RING, NS_HAND_A, NS_HAND_ACC, [ap] "+v"(ap)
                             : [bu] "n"(BU), [ac] "n"(AC), [an] "n"(AN),
                               [w0] "n"(19 - TW), [w1] "n"(18 - TW), [w2] "n"(17 - TW), [w3] "n"(16 - TW) : "memory");
            }
#undef NS_HAND_TEXT
#undef NS_XONE
#undef NS_XCNT
#undef NS_XRING
#undef NS_XS1
#undef NS_XT3
#undef NS_XFULL
#undef NS_XADD
#undef NS_XADV
#undef NS_XHALF
#undef NS_XHEAD
#undef NS_HAND_HEAD
#undef NS_HL
#undef NS_HM
#undef NS_XL
#undef NS_XLS
#undef NS_XM
        } else {
        if constexpr (BF) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Aq[U & 1][0]), "+v"(Aq[U & 1][AK - 1]) :: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Aq[U & 1][0]) :: "memory");
        a_read(Aq[(U + 1) & 1]);                   // next step's A (speculative at a run end)
        const f32x4 av = Aq[U & 1][0];
        if constexpr (BF) {
            // A rounded to bf16 where it is read: k 8 j + e of the lane's 8 (j = 0, 1: the two fragments)
            bf16x8 ab;
#pragma unroll
            for (int e = 0; e < 4; ++e) { ab[e] = (__bf16)Aq[U & 1][0][e]; ab[4 + e] = (__bf16)Aq[U & 1][AK - 1][e]; }
            if constexpr (SM) {
                // acc[4 r + c] += A(row set r, k chunk c, half h) x B(chunk c = load c, half h); ABID = block 4 c + r
                auto bf_small = [&]() {
                    const s16x4 alo = __builtin_bit_cast(s16x4, __builtin_shufflevector(ab, ab, 0, 1, 2, 3));
                    const s16x4 ahi = __builtin_bit_cast(s16x4, __builtin_shufflevector(ab, ab, 4, 5, 6, 7));
#define NS_B4(r, c, h, A4) acc[4 * (r) + (c)] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(A4, \
                __builtin_bit_cast(s16x4, __builtin_shufflevector(__builtin_bit_cast(bf16x8, Bq[U][c]), __builtin_bit_cast(bf16x8, Bq[U][c]), \
                                                                  4 * (h), 4 * (h) + 1, 4 * (h) + 2, 4 * (h) + 3)), acc[4 * (r) + (c)], 4, 4 * (c) + (r), 0);
#define NS_B4R(r, h, A4) NS_B4(r, 0, h, A4) NS_B4(r, 1, h, A4) NS_B4(r, 2, h, A4) NS_B4(r, 3, h, A4)
                    NS_B4R(0, 0, alo)
                    if constexpr (RS > 1) { NS_B4R(1, 0, alo) }
                    NS_B4R(0, 1, ahi)
                    if constexpr (RS > 1) { NS_B4R(1, 1, ahi) }
#undef NS_B4R
#undef NS_B4
                };
                if constexpr (BFT) {
                    if (si == a.nseg_f - 1) {
                        // the fp32 loss run: the fp32 engine's instructions on the unrounded first fragment (16 k per step)
#define NS_M4(r, c, e) acc[4 * (r) + (c)] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[e], Bq[U][c][e], acc[4 * (r) + (c)], 4, 4 * (c) + (r), 0);
#define NS_M4R(r, e) NS_M4(r, 0, e) NS_M4(r, 1, e) NS_M4(r, 2, e) NS_M4(r, 3, e)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            NS_M4R(0, e)
                            if constexpr (RS > 1) { NS_M4R(1, e) }
                        }
#undef NS_M4R
#undef NS_M4
                    } else {
                        bf_small();
                    }
                } else {
                    bf_small();
                }
                if constexpr (refill) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) Bq[RU][t] = wload(t);
                }
            } else {
#pragma unroll
                for (int h = 0; h < NT; h += 2) {
                    acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab, __builtin_bit_cast(bf16x8, Bq[U][h]), acc[h], 0, 0, 0);
                    acc[h + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab, __builtin_bit_cast(bf16x8, Bq[U][h + 1]), acc[h + 1], 0, 0, 0);
                    if constexpr (refill) {
                        Bq[RU][h] = wload(h);
                        Bq[RU][h + 1] = wload(h + 1);
                    }
                }
            }
        } else if constexpr (SM) {
            // acc[4 r + c] += A(rows of set r, k chunk c, element e) x B(k chunk c = load c, element e); ABID = block 4 c + r
#define NS_M4(r, c, e) acc[4 * (r) + (c)] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[e], Bq[U][c][e], acc[4 * (r) + (c)], 4, 4 * (c) + (r), 0);
#define NS_M4R(r, e) NS_M4(r, 0, e) NS_M4(r, 1, e) NS_M4(r, 2, e) NS_M4(r, 3, e)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                NS_M4R(0, e)
                if constexpr (RS > 1) { NS_M4R(1, e) }
            }
#undef NS_M4R
#undef NS_M4
            if constexpr (refill) {
#pragma unroll
                for (int t = 0; t < NT; ++t) Bq[RU][t] = wload(t);
            }
        } else {
#pragma unroll
            for (int h = 0; h < NT; h += 2) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], Bq[U][h][s], acc[h], 0, 0, 0);
                    acc[h + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], Bq[U][h + 1][s], acc[h + 1], 0, 0, 0);
                }
                if constexpr (refill) {
                    Bq[RU][h] = wload(h);
                    Bq[RU][h + 1] = wload(h + 1);
                }
            }
        }
        if constexpr (refill) wadvance();
        }
        }
        bool run_end = TX == 4;
        if constexpr (TX == 0) run_end = --kleft == 0;
        if (run_end) {
            // HAND: the run's last MFMA left the text above a few scalar instructions ago, and the compiler's hazard
            // recogniser has not seen it: sixteen wait states (eleven are required behind this 8-pass MFMA) before the
            // epilogue's vector instructions and LDS writes read the accumulators
            if constexpr (HAND) asm volatile("s_nop 15" : NS_HAND_ACC);
            // ---- end of run (si, pass).  The next segment's descriptor is requested first.  (Meant to hide under the
            // epilogue stores and the barrier; in the compiled code it does not: the descriptor's first use -- NX.type, for the
            // SIDE prefetch -- waits for it at once, ~500 cycles of scalar-cache miss per run end.  PLAIN requests it a run
            // ahead instead, plain_request.)
            const int nxi = __builtin_amdgcn_readfirstlane(min(si + 1, nseg - 1));
            const NsSeg NX = ka->seg[nxi];
            float* nx_gout = nullptr; int nx_gld = 0, nx_gn = 0;
            const float* nx_gmask = nullptr; int nx_gmld = 0;
            if constexpr (STORE) { nx_gout = ka->gout[nxi]; nx_gld = ka->gld[nxi]; nx_gn = ka->gn[nxi]; }
            if constexpr (DXE) { nx_gmask = ka->gmask[nxi]; nx_gmld = ka->gmld[nxi]; }
            int nx_gbit = -1, nx_mbit = -1;
            if constexpr (LB) { nx_gbit = ka->gbit[nxi]; nx_mbit = ka->mbit[nxi]; }
            const int cur_steps = s_steps;
            auto take_seg = [&](const NsSeg& X) {
                s_type = X.type; s_steps = X.steps; s_passes = X.passes; s_bias = X.bias_off;
                s_dst = X.dst_col; s_relu = X.relu; s_kslice = X.kslice; s_zext = X.zext; s_ncgl = X.ncg_log2; s_x0col = X.x0_col; s_x0n = X.x0_n;
                if constexpr (K4) s_kcl = X.kcl;
                if constexpr (GRAD) { s_mstore = X.mask_store; s_mapply = X.mask_apply; }
                kleft = X.steps;
            };
            auto take_next = [&]() {
                if constexpr (PLAIN) { plain_take(nxp); return; }
                take_seg(NX);
                if constexpr (STORE) { s_gout = nx_gout; s_gld = nx_gld; s_gn = nx_gn; }
                if constexpr (DXE) { s_gmask = nx_gmask; s_gmld = nx_gmld; }
                if constexpr (LB) { s_gbit = nx_gbit; s_mbit = nx_mbit; }
            };
            // SIDE segment next (and this run is its predecessor's last): its weights are requested NOW, by loads the compiler
            // does not see, so that they fly under this segment's epilogue and barrier
            f32x4 sdw[2][NT];
            bool side_next = false;
            if constexpr (K4 && !PLAIN) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int t = 0; t < NT; ++t) sdw[s2][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (NX.type == NS_SIDE && si + 1 < nseg && (s_type != NS_WIDE || pass + 1 == s_passes)) {
                    side_next = true;
                    const char* const sb = reinterpret_cast<const char*>(a.packed + NX.side_off) + (size_t)wave * NX.steps * NS_STEP_B + voff;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(sdw[0][t]) : "v"(sb + t * 1024) : "memory");
                    if (NX.steps > 1) {
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(sdw[1][t]) : "v"(sb + NS_STEP_B + t * 1024) : "memory");
                    }
                }
            }
            bool seg_done = true;
#ifdef NS_STAMPS_FINE
            const bool fine = si >= NS_STAMPS_FINE && si < NS_STAMPS_FINE + 4;
            if (fine) NS_STAMP();                  // run end reached (last MFMA issued)
#endif
            // result quads: fin[q][e] is (row, column) = SM ? (4 q + e, lane) : (4 kq + e, 16 q + li) of the wave's 64 columns
            if constexpr (SM) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = (acc[4 * q] + acc[4 * q + 1]) + (acc[4 * q + 2] + acc[4 * q + 3]);
            }
#define fin acc
#define q_row(q, e) (SM ? 4 * (q) + (e) : 4 * kq + (e))
#define q_col(q) (SM ? lane : 16 * (q) + li)
            if (s_type == NS_WIDE) {
                float* const nxt = act + (P ^ 1) * ABUF + s_dst + (!PLAIN && s_zext < 0 ? 64 * (pass ? 15 - wave : wave) : 512 * pass + 64 * wave);
                // STORE == 3, last network layer: the targets and the per-column constants of delta, fetched by inline-asm
                // loads the compiler does not count (a visible load in this loop body would turn its counted vmcnt waits
                // for the weight ring into vmcnt(0) in EVERY step); one explicit wait for all of them
                float ty[NQ][4];                        // STORE == 3: normalised targets; STORE == 2: gates
                if constexpr (STORE == 3) {
                    if (si == nlast) {
#pragma unroll
                        for (int t = 0; t < NQ; ++t) {
                            const int dc = min(512 * pass + 64 * wave + q_col(t), nout - 1);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float* py = a.t_Y + (size_t)lsrc[q_row(t, e)] * a.t_ldy + dc;
                                asm volatile("global_load_dword %0, %1, off" : "=v"(ty[t][e]) : "v"(py) : "memory");
                            }
                        }
#pragma unroll
                        for (int t = 0; t < NQ; ++t)
                            asm volatile("s_waitcnt vmcnt(0)" : "+v"(ty[t][0]), "+v"(ty[t][1]), "+v"(ty[t][2]), "+v"(ty[t][3]) :: "memory");
                    }
                }
                unsigned long long gw[SM ? NQ : 1][4];      // G2: the 64 sign bits of this wave's columns, per result row
                if constexpr (LB) {
                    if (s_mbit >= 0) {
                        const int cw = 512 * pass + 64 * wave, w0 = (s_mbit + cw) >> 5;
                        const bool mine = cw < ((s_gn + 63) & ~63);             // (past the tensor: padding columns, their gradients are zero)
#pragma unroll
                        for (int t = 0; t < (SM ? NQ : 1); ++t)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                gw[t][e] = mine ? *reinterpret_cast<const unsigned long long*>(lbits + (SM ? 4 * t + e : 4 * kq + e) * nbw + w0) : 0ull;
                    }
                }
                if constexpr (DXE && !LB) {
                    // the gates (stored forward activations), by loads the compiler does not count -- a visible load in this
                    // loop body makes every step's wait for the weight ring a vmcnt(0) -- with one explicit wait
                    if (s_gmask) {
#pragma unroll
                        for (int t = 0; t < NQ; ++t) {
                            const int mc = min(512 * pass + 64 * wave + q_col(t), s_gn - 1);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float* pg = s_gmask + (size_t)min(row0 + q_row(t, e), a.B - 1) * s_gmld + mc;
                                if constexpr (GRAD)     // written earlier in this very launch: served by the L2, not this CU's L1
                                    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(ty[t][e]) : "v"(pg) : "memory");
                                else
                                    asm volatile("global_load_dword %0, %1, off" : "=v"(ty[t][e]) : "v"(pg) : "memory");
                            }
                        }
#pragma unroll
                        for (int t = 0; t < NQ; ++t)
                            asm volatile("s_waitcnt vmcnt(0)" : "+v"(ty[t][0]), "+v"(ty[t][1]), "+v"(ty[t][2]), "+v"(ty[t][3]) :: "memory");
                    }
                }
                unsigned mbits = 0xFFFFu;
                if constexpr (GRAD) {
                    if (s_mapply) mbits = lmask[(s_mapply - 1 + pass) * (64 * NW) + threadIdx.x];   // sign bits of this very (row, col)
                    if (s_mstore) {
                        unsigned m = 0;
#pragma unroll
                        for (int t = 0; t < NQ; ++t)
#pragma unroll
                            for (int e = 0; e < 4; ++e) m |= (fin[t][e] > 0.f ? 1u : 0u) << (4 * t + e);
                        lmask[(s_mstore - 1 + pass) * (64 * NW) + threadIdx.x] = m;
                    }
                }
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // 16x16x4 C/D layout: col = lane&15, row = 4*(lane>>4) + e; 4x4x1: col = lane, row = 4 t + e
                        float v = fin[t][e];
                        if constexpr (GRAD) v = ((mbits >> (4 * t + e)) & 1u) ? v : 0.f;
                        v = s_relu ? relu_f(v) : v;
                        if constexpr (LB) {
                            if (s_mbit >= 0 && !((gw[SM ? t : 0][e] >> (SM ? lane : 16 * t + li)) & 1ull)) v = 0.f;
                        } else if constexpr (DXE) {
                            if (s_gmask && !(ty[t][e] > 0.f)) v = 0.f;
                        }
                        float v_lds = v;
                        if constexpr (STORE == 3) {
                            if (si == nlast) {                 // the network's last layer: delta replaces pred in LDS
                                const int dc = 512 * pass + 64 * wave + q_col(t);
                                const float yn = ty[t][e];
                                v_lds = dc < nout ? (isnan(yn) ? -0.f : (yn - v) + 0.f) : 0.f;   // -0: "masked", read back by the finish
                            }
                        }
                        nxt[q_row(t, e) * LD + q_col(t)] = v_lds;
                        if constexpr (LB) {
                            if (s_gbit >= 0) {                 // the sign of this activation, for the gate of its gradient
                                const unsigned long long bb = __ballot(v > 0.f);
                                const int cw = 512 * pass + 64 * wave;          // (a wave whose 64 columns lie past the tensor's
                                const bool mine = cw < ((s_gn + 63) & ~63);     //  bit range writes nothing: the next row's bits, or the
                                const int c0 = s_gbit + cw;                     //  neighbouring workgroup's LDS, sit there)
                                if constexpr (SM) {            // lane = column: 64 columns of row 4 t + e
                                    if (lane == 0 && mine) *reinterpret_cast<unsigned long long*>(lbits + (4 * t + e) * nbw + (c0 >> 5)) = bb;
                                } else {                       // 16 columns of tile t for each of the rows 4 kq + e
                                    if (li == 0 && mine) reinterpret_cast<unsigned short*>(lbits + (4 * kq + e) * nbw)[(c0 + 16 * t) >> 4] = (unsigned short)(bb >> (16 * kq));
                                }
                            }
                        }
                        if constexpr (STORE && !G2) {
                            const int grow_ = row0 + q_row(t, e), gcol = 512 * pass + 64 * wave + q_col(t);
                            if (s_gout && grow_ < a.B && gcol < s_gn) {
                                float vs = v;                      // the network's last output carries the column affine
                                if constexpr (STORE == 1)
                                    if (si == nseg - 1) vs = vs * (a.cscale ? a.cscale[gcol] : 1.f) + (a.cshift ? a.cshift[gcol] : 0.f);
                                gstore(s_gout + (size_t)grow_ * s_gld + gcol, vs);
                            }
                        }
                    }
#ifdef NS_STAMPS_FINE
                if (fine) NS_STAMP();              // epilogue done (LDS writes and stores issued)
#endif
                if (++pass == s_passes) {
                    lds_barrier();
                    NS_STAMP();
                    P ^= 1; pass = 0; ++si;
                    take_next();
                } else {
                    kleft = !PLAIN && s_zext > 0 ? s_zext : cur_steps;    // (a short second pass: NsSeg::zext)
                    seg_done = false;
                }
            } else {
                // [8 waves][ROWS][64 cols]; the column is swizzled per row so that the reduce below reads without bank
                // conflicts: col ^= 16*(row>>2) (16 rows), col ^= 32*(row&1) (4x4x1 engines)
                float* const part = act + (P ^ 1) * ABUF;
                constexpr int PW = ROWS * 64;
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int rr = q_row(t, e);
                        part[wave * PW + rr * 64 + (q_col(t) ^ (SM ? 32 * (rr & 1) : 16 * kq))] = fin[t][e];
                    }
#ifdef NS_STAMPS_FINE
                if (fine) NS_STAMP();              // partials written (issued)
#endif
                lds_barrier();
#ifdef NS_STAMPS_FINE
                if (fine) NS_STAMP();              // first barrier passed
#endif
                // thread (row sr, lane sc0 of RGS): columns sc0, sc0+RGS, ...; wave of (K part kp, group cg) = kp*ncg + cg.
                // 16 rows: the prologue's 32 threads per row; 8 / 4 rows: ALL 512 threads, 64 / 128 per row (with 32 per row
                // three quarters of a 4-row workgroup watched the other quarter reduce)
                constexpr int RGS = SM ? 64 * NW / ROWS : RG;
                const int sr = SM ? tid / RGS : pr, sc0 = SM ? tid % RGS : pc0;
                const bool srow = SM ? true : prow;
                float* const cur = act + P * ABUF + sr * LD + s_dst;
                const int ncol = 64 << s_ncgl, nkp = NW >> s_ncgl;
                const int sw = SM ? 32 * (sr & 1) : 16 * (sr >> 2);
                constexpr int NGJ = 256 / RGS;          // (SPLIT outputs are <= 256 columns: 8 / 4 / 2 per thread)
                float sg[NGJ];
                if constexpr (DXE && !LB) {
                    if (s_gmask) {
#pragma unroll
                        for (int j = 0; j < NGJ; ++j) {
                            const float* pg = s_gmask + (size_t)min(row0 + sr, a.B - 1) * s_gmld + min(sc0 + RGS * j, s_gn - 1);
                            if constexpr (GRAD)
                                asm volatile("global_load_dword %0, %1, off sc1" : "=v"(sg[j]) : "v"(pg) : "memory");
                            else
                                asm volatile("global_load_dword %0, %1, off" : "=v"(sg[j]) : "v"(pg) : "memory");
                        }
#pragma unroll
                        for (int j = 0; j < NGJ; ++j) asm volatile("s_waitcnt vmcnt(0)" : "+v"(sg[j]) :: "memory");
                    }
                }
                int gj = 0;
                if constexpr ((!LB && !DXE && !STORE) || (LB && !SM)) {
                    // serving (and the one-launch gradient on the 16-row engine): FOUR adjacent columns per thread and trip, as 16-byte LDS accesses (the swizzle moves whole groups of
                    // 16 / 32 columns, the biases start at multiples of 64): a quarter of the LDS instructions of the column-per-
                    // trip loop below, and all K parts of a trip in flight -- 256 output columns were 8 trips of ~130 cycles
                    // each behind the barrier.  The sums in the order of the loop below.
                    auto reduce4 = [&](auto NKc) {
                        constexpr int NK = decltype(NKc)::value;
                        for (int c = 4 * sc0; c < (srow ? s_zext : 0); c += 4 * RGS) {
                            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                            if (c < ncol) {
                                const float* src = part + (c >> 6) * PW + sr * 64 + ((c & 63) ^ sw);
                                constexpr int CH = LB && NK > 4 ? 4 : NK;        // K parts in flight (the gradient launch has no 32 registers to spare)
                                const f32x4 b = *reinterpret_cast<const f32x4*>(lbias + s_bias + c);
#pragma unroll
                                for (int k0 = 0; k0 < NK; k0 += CH) {
                                    f32x4 x[CH];
#pragma unroll
                                    for (int kp = 0; kp < CH; ++kp) x[kp] = *reinterpret_cast<const f32x4*>(src + ((k0 + kp) << s_ncgl) * PW);
#pragma unroll
                                    for (int kp = 0; kp < CH; ++kp) v += x[kp];
                                }
                                v += b;
                                if (s_relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                            }
                            if constexpr (LB) {
                                // the gate: four sign bits of the tensor this gradient belongs to (bit columns s_mbit + c ..; c & 31 <= 28)
                                const bool mine = c < ((s_gn + 63) & ~63);
                                if (s_mbit >= 0) {
                                    const unsigned nib = mine ? (lbits[sr * nbw + ((s_mbit + c) >> 5)] >> (c & 31)) & 0xFu : 0u;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] = ((nib >> e) & 1u) ? v[e] : 0.f;
                                }
                                *reinterpret_cast<f32x4*>(cur + c) = v;
                                if (s_gbit >= 0) {
                                    // the signs of these activations: the eight threads of a 32-column word OR their nibbles together
                                    unsigned w32 = ((v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u)) << (c & 31);
                                    w32 |= __shfl_xor(w32, 1, 64); w32 |= __shfl_xor(w32, 2, 64); w32 |= __shfl_xor(w32, 4, 64);
                                    if ((sc0 & 7) == 0 && mine) lbits[sr * nbw + ((s_gbit + c) >> 5)] = w32;
                                }
                            } else {
                                *reinterpret_cast<f32x4*>(cur + c) = v;
                            }
                        }
                    };
                    if (nkp == NW) reduce4(std::integral_constant<int, NW>{});
                    else if (nkp == NW / 2) reduce4(std::integral_constant<int, NW / 2>{});
                    else reduce4(std::integral_constant<int, 2>{});
                } else
                for (int c = sc0; c < (srow ? s_zext : 0); c += RGS, ++gj) {
                    float v = 0.f;
                    if (c < ncol) {
                        const float* src = part + (c >> 6) * PW + sr * 64 + ((c & 63) ^ sw);
                        // the partials of this column's K parts, all reads in flight (8, 4 or 2 of them: the same sums in the
                        // same order as one loop over kp < nkp)
                        if (nkp == NW) {
                            float x[NW];
#pragma unroll
                            for (int kp = 0; kp < NW; ++kp) x[kp] = src[(kp << s_ncgl) * PW];
#pragma unroll
                            for (int kp = 0; kp < NW; ++kp) v += x[kp];
                        } else if (nkp == NW / 2) {
                            float x[NW / 2];
#pragma unroll
                            for (int kp = 0; kp < NW / 2; ++kp) x[kp] = src[(kp << s_ncgl) * PW];
#pragma unroll
                            for (int kp = 0; kp < NW / 2; ++kp) v += x[kp];
                        } else {
                            const float x0 = src[0], x1 = src[(1 << s_ncgl) * PW];
                            v += x0; v += x1;
                        }
                        v += lbias[s_bias + c];
                        if (s_relu) v = relu_f(v);
                        if constexpr (LB) {
                            if (s_mbit >= 0 && !(c < ((s_gn + 63) & ~63) && ((lbits[sr * nbw + ((s_mbit + c) >> 5)] >> (c & 31)) & 1u))) v = 0.f;
                        } else if constexpr (DXE) {
                            float gv = 1.f;             // (dynamic register-array index: a select chain)
#pragma unroll
                            for (int j = 0; j < NGJ; ++j) gv = gj == j ? sg[j] : gv;
                            if (s_gmask && !(gv > 0.f)) v = 0.f;
                        }
                        if constexpr (STORE && !G2) {
                            if (s_gout && row0 + sr < a.B && c < s_gn) {
                                float vs = v;
                                if constexpr (STORE == 1)
                                    if (si == nseg - 1) vs = vs * (a.cscale ? a.cscale[c] : 1.f) + (a.cshift ? a.cshift[c] : 0.f);
                                gstore(s_gout + (size_t)(row0 + sr) * s_gld + c, vs);
                            }
                        }
                    }
                    cur[c] = v;
                    if constexpr (LB) {
                        if (s_gbit >= 0) {                  // (every lane of a wave runs the same trips of this loop)
                            const unsigned long long bb = __ballot(v > 0.f);
                            const bool mine = c < ((s_gn + 63) & ~63);
                            if constexpr (SM) { if (lane == 0 && mine) *reinterpret_cast<unsigned long long*>(lbits + sr * nbw + ((s_gbit + c) >> 5)) = bb; }
                            else { if ((lane & 31) == 0 && mine) lbits[sr * nbw + ((s_gbit + c) >> 5)] = (unsigned)(bb >> (lane & 32)); }
                        }
                    }
                }
                if constexpr (STORE == 3) {
                    if (si == nlast) {
                        // the network's last layer (nout <= 256): thread (row sr, lane sc0) turns its own columns
                        // sc0 + RGS j of pred into delta, in place (asm loads: see the WIDE epilogue)
                        constexpr int NJ = NGJ;
                        const int ysrc = lsrc[sr];
                        float sy[NJ];
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int c = min(sc0 + RGS * j, nout - 1);
                            asm volatile("global_load_dword %0, %1, off" : "=v"(sy[j]) : "v"(a.t_Y + (size_t)ysrc * a.t_ldy + c) : "memory");
                        }
#pragma unroll
                        for (int j = 0; j < NJ; ++j) asm volatile("s_waitcnt vmcnt(0)" : "+v"(sy[j]) :: "memory");
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int c = sc0 + RGS * j;
                            if (c < nout && srow) cur[c] = isnan(sy[j]) ? -0.f : (sy[j] - cur[c]) + 0.f;
                        }
                    }
                }
#ifdef NS_STAMPS_FINE
                if (fine) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); NS_STAMP(); }   // reduce done
#endif
                lds_barrier();
                NS_STAMP();
                ++si;
                take_next();
            }
            if constexpr (GRAD) {
                if (seg_done && si == a.nseg_f) {   // (seg_done: not again after a pass of the first backward segment)
                    if constexpr (DXE && !LB)       // the forward activations every wave stored are in memory before any gate load
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if constexpr (TRB) {
                        // ---- turnaround of a training step = the loss finish: delta and U = delta Cinv sit in LDS (U at column
                        // u_col of buffer P, or at column 0 with delta in the other buffer).  loss_b = delta . U / den
                        // (util.py:1086-1088); d loss / d pred = -2 U inv_batch / den, zero where delta was masked, goes to
                        // memory (the last layer's parameter gradient reads it) AND over delta / U in LDS: the input rows of the
                        // first backward segment (their padding columns hold the zeros the forward left there).
                        {
                            const float* const F = act + P * ABUF + pr * LD;
                            const bool rok = prow && row0 + pr < a.B;
                            const float* const Dv = a.u_same ? F : act + (P ^ 1) * ABUF + pr * LD;
                            const float* const Uv = a.u_same ? F + a.u_col : F;
                            float chi = 0.f;
                            for (int c = pc0; c < nout; c += RG) chi += Dv[c] * Uv[c];
#pragma unroll
                            for (int o = RG / 2; o >= 1; o >>= 1) chi += __shfl_xor(chi, o, 64);
                            if (rok && pc0 == 0) gstore(a.t_loss_rows + row0 + pr, chi / lden[pr]);
                        }
                        lds_barrier();                  // every row's chi is taken before delta is overwritten (u_same)
                        {
                            constexpr int TPR = 64 * NW / ROWS;
                            const int fr = tid / TPR, fc = tid % TPR;
                            float* const Fr = act + P * ABUF + fr * LD;
                            const float* const Dr = a.u_same ? Fr : act + (P ^ 1) * ABUF + fr * LD;
                            const float* const Ur = a.u_same ? Fr + a.u_col : Fr;
                            const float dr = lden[fr];
                            const bool rowok = row0 + fr < a.B;
                            for (int c = fc; c < a.t_lddp; c += TPR) {
                                float g = 0.f;
                                if (c < nout && rowok) {
                                    const bool masked = __float_as_uint(Dr[c]) == 0x80000000u;
                                    g = masked ? 0.f : (-2.f * Ur[c]) * a.t_inv_batch / dr;
                                }
                                if (rowok) gstore(a.t_dP + (size_t)(row0 + fr) * a.t_lddp + c, g);
                                if (c < nout) Fr[c] = g;
                            }
                        }
                        lds_barrier();
                    } else if constexpr (DGR) {
                        // ---- turnaround behind the dense segment (an instantiation of its own): U = d L sits at column u_col of
                        // buffer P behind d (u_same), or at column 0 with d in the other buffer.  chi2 = sum U_c^2 -- the factored
                        // form linna_logprob_eval serves -- and d lnP / dU_c = -U_c / T goes to column c of buffer P, the input of
                        // the transposed dense map: over d (which nothing reads again) or over U itself, every thread its own
                        // columns.  The columns past nout meet zero weights there.
                        float* const F = act + P * ABUF + pr * LD;
                        const float* const U = a.u_same ? F + a.u_col : F;
                        float chi = 0.f;
                        if (prow)
                            for (int c = pc0; c < nout; c += RG) {
                                const float u = U[c];
                                chi += u * u;
                                F[c] = -u / a.T;
                            }
#pragma unroll
                        for (int o = RG / 2; o >= 1; o >>= 1) chi += __shfl_xor(chi, o, 64);
                        lnp_grad = (-0.5f * chi) / a.T + (-0.5f * zz);
                        lds_barrier();
                    } else {
                    // ---- turnaround: the output rows (bias added) sit in buffer P.  lnP as in the finish, and
                    // d lnP / d out = -(d w) gscale / T written over them: the input of the first backward segment
                    float* const F = act + P * ABUF + pr * LD;
                    float chi = 0.f;
#pragma unroll
                    for (int i = 0; i < FIN; ++i) {
                        const int c = pc0 + i * RG;
                        if (c < nout && prow) {
                            const float d = F[c] * fcs[i] + fct[i];
                            chi += (d * fw[i]) * d;
                            F[c] = -(d * fw[i]) * fgs[i] / a.T;
                        }
                    }
                    if constexpr (WOUT) {
                        // wide outputs (an instantiation of its own, as EPS is): the columns past the FIN register-held ones,
                        // their constants straight from memory -- here in the turnaround, once per launch, outside `step`
                        if (prow)
                            for (int c = pc0 + FIN * RG; c < nout; c += RG) {
                                const float d = F[c] * (a.cscale ? a.cscale[c] : 1.f) + (a.cshift ? a.cshift[c] : 0.f);
                                const float dw = d * a.w[c];
                                chi += dw * d;
                                F[c] = -dw * a.gscale[c] / a.T;
                            }
                    }
#pragma unroll
                    for (int o = RG / 2; o >= 1; o >>= 1) chi += __shfl_xor(chi, o, 64);
                    lnp_grad = (-0.5f * chi) / a.T + (-0.5f * zz);
                    lds_barrier();
                    }
                }
            }
#undef fin
#undef q_row
#undef q_col
            if (!PLAIN && seg_done && si < nseg && s_x0col > 0) {
                // input skip: the kept input rows go behind this segment's regular input (one GEMM over [h ; x0])
                if (prow) {
                    float* const dstp = act + P * ABUF + pr * LD + s_x0col;
#pragma unroll
                    for (int i = 0; i < ZPRE; ++i)
                        if (pc0 + i * RG < s_x0n) dstp[pc0 + i * RG] = lx0[pr * 64 + pc0 + i * RG];
                }
                lds_barrier();
            }
            if constexpr (K4 && !PLAIN) {
                if (side_next && seg_done) {
                    // ---- SIDE run: the segment now in s_* (taken above), whole, right here.  Wave w owns the k range
                    // [w kslice, (w + 1) kslice) (ncg = 1); a step covers kc chunks of 16 k: tile t of the weights is
                    // (column tile t % (4 / kc), chunk t / (4 / kc)).
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const bool kc4 = s_kcl == 2, kc1 = s_kcl == 0;
                    const uint32_t abase = act_lds + 4u * (uint32_t)(P * ABUF + li * LD + 4 * kq + wave * s_kslice);
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        if (s2 < s_steps) {
                            const uint32_t as = abase + (uint32_t)s2 * (64u << s_kcl);
                            f32x4 af0, af1, af2 = f32x4{0.f, 0.f, 0.f, 0.f}, af3 = f32x4{0.f, 0.f, 0.f, 0.f};
                            asm volatile("ds_read_b128 %0, %1" : "=v"(af0) : "v"(as) : "memory");
                            af1 = f32x4{0.f, 0.f, 0.f, 0.f};
                            if (!kc1) asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(af1) : "v"(as) : "memory");
                            if (kc4) {
                                asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(af2) : "v"(as) : "memory");
                                asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(af3) : "v"(as) : "memory");
                            }
                            if (s2 == 0)
                                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                                             : "+v"(af0), "+v"(af1), "+v"(af2), "+v"(af3), "+v"(sdw[0][0]), "+v"(sdw[0][1]), "+v"(sdw[0][2]),
                                               "+v"(sdw[0][3]), "+v"(sdw[1][0]), "+v"(sdw[1][1]), "+v"(sdw[1][2]), "+v"(sdw[1][3]) :: "memory");
                            else
                                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af0), "+v"(af1), "+v"(af2), "+v"(af3) :: "memory");
                            // tile t multiplies chunk t (kc = 4), t >> 1 (kc = 2) or the one chunk (kc = 1)
                            const f32x4 f1 = kc4 ? af1 : af0, f2 = kc4 ? af2 : kc1 ? af0 : af1, f3 = kc4 ? af3 : kc1 ? af0 : af1;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(af0[e], sdw[s2][0][e], acc[0], 0, 0, 0);
                                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1[e], sdw[s2][1][e], acc[1], 0, 0, 0);
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(f2[e], sdw[s2][2][e], acc[2], 0, 0, 0);
                                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(f3[e], sdw[s2][3][e], acc[3], 0, 0, 0);
                            }
                        }
                    }
                    int treal = NT;
                    if (kc4) { acc[0] = (acc[0] + acc[1]) + (acc[2] + acc[3]); treal = 1; }
                    else if (!kc1) { acc[0] = acc[0] + acc[2]; acc[1] = acc[1] + acc[3]; treal = 2; }
                    float* const part = act + (P ^ 1) * ABUF;       // [8 waves][16 rows][64]: the SPLIT layout and swizzle
                    constexpr int PW = ROWS * 64;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < treal) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) part[wave * PW + (4 * kq + e) * 64 + ((16 * t + li) ^ (16 * kq))] = acc[t][e];
                        }
#ifdef NS_STAMPS_FINE
                    if (fine) NS_STAMP();          // SIDE: MFMAs issued, partials written
#endif
                    lds_barrier();
#ifdef NS_STAMPS_FINE
                    if (fine) NS_STAMP();          // SIDE: first barrier passed
#endif
                    {                                  // four adjacent columns per thread, 16-byte accesses: the SPLIT reduce's form
                        float* const cur = act + P * ABUF + pr * LD + s_dst;
                        const int ncol = 16 * treal, sw = 16 * (pr >> 2);
                        for (int c = 4 * pc0; c < s_zext; c += 4 * RG) {
                            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                            if (c < ncol) {
                                const float* src = part + pr * 64 + (c ^ sw);
                                constexpr int CH = LB ? 4 : NW;
                                const f32x4 b = *reinterpret_cast<const f32x4*>(lbias + s_bias + c);
#pragma unroll
                                for (int k0 = 0; k0 < NW; k0 += CH) {
                                    f32x4 x[CH];
#pragma unroll
                                    for (int kp = 0; kp < CH; ++kp) x[kp] = *reinterpret_cast<const f32x4*>(src + (k0 + kp) * PW);
#pragma unroll
                                    for (int kp = 0; kp < CH; ++kp) v += x[kp];
                                }
                                v += b;
                                if (s_relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                            }
                            if constexpr (LB) {         // a backward SIDE segment (d/dh) is gated by the sign bits of h; a forward one records them
                                const bool mine = c < ((s_gn + 63) & ~63);
                                if (s_mbit >= 0) {
                                    const unsigned nib = mine ? (lbits[pr * nbw + ((s_mbit + c) >> 5)] >> (c & 31)) & 0xFu : 0u;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] = ((nib >> e) & 1u) ? v[e] : 0.f;
                                }
                                *reinterpret_cast<f32x4*>(cur + c) = v;
                                if (s_gbit >= 0) {
                                    unsigned w32 = ((v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u)) << (c & 31);
                                    w32 |= __shfl_xor(w32, 1, 64); w32 |= __shfl_xor(w32, 2, 64); w32 |= __shfl_xor(w32, 4, 64);
                                    if ((pc0 & 7) == 0 && mine) lbits[pr * nbw + ((s_gbit + c) >> 5)] = w32;
                                }
                            } else {
                                *reinterpret_cast<f32x4*>(cur + c) = v;
                            }
                        }
                    }
#ifdef NS_STAMPS_FINE
                    if (fine) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); NS_STAMP(); }   // SIDE: reduce done
#endif
                    lds_barrier();
                    NS_STAMP();
                    ++si;
                    const int n2i = __builtin_amdgcn_readfirstlane(min(si, nseg - 1));
                    const NsSeg N2 = ka->seg[n2i];
                    take_seg(N2);
                    if constexpr (LB) { s_gbit = ka->gbit[n2i]; s_mbit = ka->mbit[n2i]; s_gn = ka->gn[n2i]; }
                }
            }
            if (si < nseg) {
                begin_run();
                if constexpr (TX == 4) {
                    // (the slot's parity is a run-time value here: the run's first fragment goes into BOTH fragments' registers
                    // -- the one the step behind read is dead, and the next step's own A read overwrites it in LDS order)
                    asm volatile("ds_read_b128 v[224:227], %2\n\tds_read_b128 v[228:231], %2"
                                 : "={v[224:227]}"(Aq[0][0]), "={v[228:231]}"(Aq[1][0]) : "v"(ap) : "memory");
                    ap += 64;
                } else
                a_read(Aq[(U + 1) & 1]);           // replaces the speculative fragment
                if constexpr (PLAIN) { if (seg_done) plain_request(); }
            }
#ifdef NS_STAMPS_FINE
            if (fine) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); NS_STAMP(); }   // next run ready to issue
#endif
        }
    };
    using T_ = std::true_type; using F_ = std::false_type;
    using X0_ = std::integral_constant<int, 0>;
#define NS_STEP(U, RF) if constexpr (U < R) step(std::integral_constant<int, U>{}, RF{}, X0_{});
    const int ngroups = a.G / R, rem = a.G - ngroups * R;
    if constexpr (TRIM) {
        // The trimmed launch: one statement for every step (TX == 5) and ONE copy of the run end.  A run is one pass through
        // that statement -- the full text, or T3 where the wave's fourth tile is padding -- but for the last step of a run
        // whose K ends one k into it: the S1 step, a pass of its own.  s_trim holds both choices (set in begin_run).  Every
        // step refills (past the stream's end its last step again, never used), so every wait finds the twenty loads in
        // flight it counts on.
        const int G = a.G;
        int g = 0;
#pragma unroll 1
        while (g < G) {
            const int n = __builtin_amdgcn_readfirstlane((s_trim & 2) ? kleft - 1 : kleft);     // (0: the S1 step alone)
            s_n = n;
            s_tx = s_trim & 1;
            step(X0_{}, T_{}, std::integral_constant<int, 5>{});
            const int done = n ? n : 1;
            g += done; kleft -= done; s_sel = (s_sel + done) % R;
            if (kleft == 0) step(X0_{}, T_{}, std::integral_constant<int, 4>{});
        }
    } else {
#pragma unroll 1
    for (int it = 0; it < ngroups; ++it) {
        NS_STEP(0, T_) NS_STEP(1, T_) NS_STEP(2, T_) NS_STEP(3, T_) NS_STEP(4, T_) NS_STEP(5, T_) NS_STEP(6, T_) NS_STEP(7, T_)
    }
#define NS_TAIL(U) if constexpr (U < R - 1) { if (rem > U) step(std::integral_constant<int, U>{}, F_{}, X0_{}); }
    NS_TAIL(0) NS_TAIL(1) NS_TAIL(2) NS_TAIL(3) NS_TAIL(4) NS_TAIL(5) NS_TAIL(6)
#undef NS_TAIL
    }
#undef NS_STEP
    // The last speculative A read.  Both fragments are operands of the wait: the compiler does not know that the
    // inline-asm ds_read lands later, and a fragment nobody reads again would otherwise be dead at once -- its
    // registers could be handed to an accumulator of the final step, which the returning LDS data then overwrites.
    if constexpr (BF) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Aq[0][0]), "+v"(Aq[0][AK - 1]), "+v"(Aq[1][0]), "+v"(Aq[1][AK - 1]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Aq[0][0]), "+v"(Aq[1][0]) :: "memory");
    NS_STAMP();

    if constexpr (((STORE == 1 || STORE == 2) && !GRAD) || TRB) { NS_STAMPS_FLUSH(); return; }   // every output is in global memory already
    if constexpr (STORE == 3) {
        // ---- 5 (loss).  delta and U = delta Cinv sit in LDS (as d and U of the dense serving program): chi2 = delta . U,
        // loss_b = chi2 / den (util.py:1086-1088), d loss / d pred = -2 U inv_batch / den, zero where delta was masked
        const float* const F = act + P * ABUF + pr * LD;
        const bool rok = prow && row0 + pr < a.B;
        const float* const Dv = a.u_same ? F : act + (P ^ 1) * ABUF + pr * LD;
        const float* const Uv = a.u_same ? F + a.u_col : F;
        float chi = 0.f;
        for (int c = pc0; c < nout; c += RG) chi += Dv[c] * Uv[c];
#pragma unroll
        for (int o = RG / 2; o >= 1; o >>= 1) chi += __shfl_xor(chi, o, 64);
        if (rok && pc0 == 0) a.t_loss_rows[row0 + pr] = chi / lden[pr];
        {
            // d loss / d pred by ALL threads of the workgroup, 512 / ROWS per row (the row's 32 threads alone walked a
            // 457-wide row in 15 rounds while three quarters of the workgroup waited: 8 k cycles at the kernel's tail)
            constexpr int TPR = 64 * NW / ROWS;
            const int fr = tid / TPR, fc = tid % TPR;
            if (row0 + fr < a.B) {
                const float* const Fr = act + P * ABUF + fr * LD;
                const float* const Dr = a.u_same ? Fr : act + (P ^ 1) * ABUF + fr * LD;
                const float* const Ur = a.u_same ? Fr + a.u_col : Fr;
                const float dr = lden[fr];
                for (int c = fc; c < a.t_lddp; c += TPR) {
                    float g = 0.f;
                    if (c < nout) {
                        const bool masked = __float_as_uint(Dr[c]) == 0x80000000u;
                        g = masked ? 0.f : (-2.f * Ur[c]) * a.t_inv_batch / dr;
                    }
                    a.t_dP[(size_t)(row0 + fr) * a.t_lddp + c] = g;
                }
            }
        }
        NS_STAMP();
        NS_STAMPS_FLUSH();
        return;
    }
    // ---- 5 (GRAD). d lnP / d x sits in buffer P: the derivative of the input transform and of the prior map
    // (util.py:339-347, 483-497), minus z for the Gaussian prior term; lnP from the turnaround
    if constexpr (GRAD) {
        const float* const F = act + P * ABUF + pr * LD;
        const bool rok = prow && row0 + pr < a.B;
        if (rok) {
            // the leapfrog's step sizes: the launch's own, or -- EPS, an instantiation of its own -- the multipliers of this
            // row's (a chain's adapted step size).  A run-time test of a.hm_eps here cost the launches WITHOUT one 0.3-0.5 us:
            // its argument loads were hoisted into a prologue that has no scalar register left (DESIGN 3.10).
            float hm_ek = a.hm_ek, hm_ed = a.hm_ed;
            if constexpr (EPS) { const float e = a.hm_eps[row0 + pr]; hm_ek *= e; hm_ed *= e; }
#pragma unroll
            for (int j = 0; j < ZPRE; ++j) {
                const int c = pc0 + j * RG;
                if (c < nin) {
                    float g = F[c] / zxs[j];
                    if (a.lg && zlg[j]) g = g / (theta[j] * 2.30258509299404568f);
                    const float z = zr[j];
                    const float dth = zfl[j] ? za2[j] * (expf(-0.5f * z * z) * 0.398942280401432678f) : za2[j];
                    const float gz = g * dth - z;
                    a.Gout[(size_t)(row0 + pr) * a.ldg + c] = gz;
                    if (a.hm_p) {
                        // the leapfrog's kick with this gradient and the drift to the next position (hmc_kick_drift_kernel's
                        // arithmetic: the launch between two gradient evaluations it replaces was 4.5 us of nothing)
                        float* const pp = a.hm_p + (size_t)(row0 + pr) * a.hm_ldp + c;
                        float pm = *pp;
                        if (a.hm_ek != 0.f) { pm += hm_ek * gz; *pp = pm; }
                        if (a.hm_ed != 0.f) a.hm_q[(size_t)(row0 + pr) * a.ldz + c] = z + hm_ed * (pm / a.hm_mass[c]);
                    }
                }
            }
            if (pc0 == 0) a.lnP[row0 + pr] = isnan(lnp_grad) ? -INFINITY : lnp_grad;
        }
        if constexpr (STORE == 2) { NS_STAMP(); NS_STAMPS_FLUSH(); }     // (diagnostic build; the MLP-only GRAD keeps its masks where the stamps would sit)
        return;
    }
    // ---- 5. output rows are in buffer P (bias added, no ReLU): output transform, d, log-likelihood
    // (PLAIN: the launcher has checked that there is no exp map, no dense segment, no D / TH output, and that cscale,
    // cshift, w and lnP are all there -- every test of them below is decided at compile time)
    {
        const float* const F = act + P * ABUF + pr * LD;
        const bool rok = prow && row0 + pr < a.B;
        float chi = 0.f;
        auto column = [&](int c, float cs, float ct, float ww) {
            float d = F[c] * cs + ct;
            if (!PLAIN && a.cpost) d = expf(d) * a.cpost[c] + a.cshift2[c];
            if (!PLAIN && a.D && rok) a.D[(size_t)(row0 + pr) * a.ldd + c] = isnan(zz) ? zz : d;   // (a poisoned row stays one for a later likelihood launch)
            chi += (d * ww) * d;
        };
        if (!PLAIN && a.dense) {
            // the last segment multiplied d (output map folded into the last layer) by the dense inverse covariance
            const float* const Dv = a.u_same ? F : act + (P ^ 1) * ABUF + pr * LD;
            const float* const U = a.u_same ? F + a.u_col : F;
            const bool fac = a.dense == 2;      // the segment multiplied by L (S = L L^T): chi2 = |d L|^2, a sum of squares
            for (int c = pc0; c < nout; c += RG) {
                const float d = Dv[c];
                if (a.D && rok) a.D[(size_t)(row0 + pr) * a.ldd + c] = isnan(zz) ? zz : d;
                const float u = U[c];
                chi += (fac ? u : d) * u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < FIN; ++i)
                if (pc0 + i * RG < nout) column(pc0 + i * RG, fcs[i], fct[i], fw[i]);
            for (int c = pc0 + FIN * RG; c < nout; c += RG)        // wide outputs: constants straight from memory
                column(c, PLAIN || a.cscale ? a.cscale[c] : 1.f, PLAIN || a.cshift ? a.cshift[c] : 0.f, PLAIN || a.w ? a.w[c] : 0.f);
        }
#pragma unroll
        for (int o = RG / 2; o >= 1; o >>= 1) chi += __shfl_xor(chi, o, 64);
        float lnp_new = (-0.5f * chi) / a.T + (-0.5f * zz);
        lnp_new = isnan(lnp_new) ? -INFINITY : lnp_new;
        if constexpr (MOVE == 2) {
            if (a.lnP && pc0 == 0 && prow && row0 + pr < mv_rows) a.lnP[a.mv_C ? grow : row0 + pr] = lnp_new;
        } else {
            if ((PLAIN || (a.lnP && (a.w || a.dense))) && pc0 == 0 && rok) a.lnP[row0 + pr] = lnp_new;
        }
        if constexpr (MOVE == 1) {
            // Metropolis test of the stretch move (linna_stretch_accept); every lane of the row agrees
            const bool mv_acc = rok && mv_factor + lnp_new - mv_lnp_old > mv_logu;
            if (mv_acc) {
#pragma unroll
                for (int j = 0; j < ZPRE; ++j)
                    if (pc0 + j * RG < nin) a.mv_coords[(size_t)mv_wk * a.mv_ldc + pc0 + j * RG] = zr[j];
                if (pc0 == 0) {
                    a.mv_logp[mv_wk] = lnp_new;
                    if (a.mv_naccept) a.mv_naccept[mv_wk] += 1;
                }
            }
            if (a.mv_chain && rok) {
                // the walker's position after this iteration goes straight into the chain block (a walker moves in ONE of the
                // two half steps of an iteration: the two launches together fill the row)
#pragma unroll
                for (int j = 0; j < ZPRE; ++j)
                    if (pc0 + j * RG < nin)
                        a.mv_chain[(size_t)mv_wk * nin + pc0 + j * RG] = mv_acc ? zr[j] : a.mv_coords[(size_t)mv_wk * a.mv_ldc + pc0 + j * RG];
                if (pc0 == 0) a.mv_lps[mv_wk] = mv_acc ? lnp_new : mv_lnp_old;
            }
        }
        if (!PLAIN && a.TH && rok) {
#pragma unroll
            for (int j = 0; j < ZPRE; ++j)
                if (pc0 + j * RG < nin) a.TH[(size_t)(row0 + pr) * a.ldt + pc0 + j * RG] = theta[j];
            for (int c = pc0 + ZPRE * RG; c < nin; c += RG)     // wide inputs: theta recomputed rather than kept
                a.TH[(size_t)(row0 + pr) * a.ldt + c] = ns_prior_theta(a.Z[(size_t)grow * a.ldz + c], a.is_flat[c], a.a1[c], a.a2[c]);
        }
    }
    // HAND: the last refills (the stream's last step again, never used) may still be on their way into the ring, and the
    // compiler knows of no load: the ring stays an operand to the end, so that the finish above was given none of its registers
    if constexpr (HAND) asm volatile("" : NS_HAND_RING);
    NS_STAMP();
    NS_STAMPS_FLUSH();
#undef NS_STAMP
#undef NS_STAMPS_FLUSH
#undef NS_HAND_RING
#undef NS_HAND_A
#undef NS_HAND_ACC
