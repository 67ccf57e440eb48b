// Op-level and debug entry points of the C ABI (include/mi355ppo.h): single kernels and small launch sequences on caller data, for
// tests and micro-benchmarks.  The production launch path (engine.hip) never goes through here.
#include "engine_ctx.h"

static int shape_of(int cin, int cout, int hw, ConvShape* s) {
    for (int k = 0; k < CS_COUNT; ++k) {
        int a, b, h; conv_shape_dims((ConvShape)k, &a, &b, &h);
        if (a == cin && b == cout && h == hw) { *s = (ConvShape)k; return 0; }
    }
    return fail(-1, "unsupported conv shape");
}

// host-side activation conversion for the op-level entry points of a bf16 context (round to nearest even; mi_create builds its uint8 -> bf16 table with it)
std::vector<uint16_t> host_to_bf16(const float* x, size_t n) {
    std::vector<uint16_t> o(n);
    for (size_t k = 0; k < n; ++k) { uint32_t u; memcpy(&u, x + k, 4); o[k] = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }
    return o;
}
static void host_from_bf16(const uint16_t* h, float* x, size_t n) {
    for (size_t k = 0; k < n; ++k) { const uint32_t u = ((uint32_t)h[k]) << 16; memcpy(x + k, &u, 4); }
}
// Device memory of one op-level call.  Every buffer is freed on every return path.  Outputs the kernels write are poisoned with
// 0xFF bytes (NaN in bf16 and fp32), so an element a kernel skips reads back as NaN; the targets the slab reduction adds into keep
// a zero fill.  A canary band follows each output (and covers the weight-gradient slab rows past a launch's grid); check() compares
// the bands after the launch and names the tensor a kernel wrote past.  The bands sit after the tensors only: bases keep hipMalloc's
// alignment.  The production launch path never goes through here.
struct OpMem {
    static constexpr size_t GUARD = 64 * 1024;
    static constexpr int CANARY = 0xA5;
    struct Band { std::string name; unsigned char* p; size_t bytes; bool rezero; };
    const char* hook; hipStream_t st;
    std::vector<void*> owned;
    std::vector<Band> bands;
    OpMem(const char* h, hipStream_t s) : hook(h), st(s) {}
    ~OpMem() { for (void* p : owned) hipFree(p); }
    OpMem(const OpMem&) = delete;
    OpMem& operator=(const OpMem&) = delete;
    template <typename T>
    hipError_t alloc(T** p, size_t bytes) {          // an input: the +256 bytes cover the kernels' vector over-reads
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes + 256);
        if (e != hipSuccess) return e;
        owned.push_back(q); *p = (T*)q;
        return hipMemsetAsync(q, 0, bytes + 256, st);
    }
    template <typename T>
    hipError_t out(T** p, size_t bytes, const char* name, int fill = 0xFF) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes + GUARD);
        if (e != hipSuccess) return e;
        owned.push_back(q); *p = (T*)q;
        if ((e = hipMemsetAsync(q, fill, bytes, st)) != hipSuccess) return e;
        return band((unsigned char*)q + bytes, GUARD, name, false);
    }
    // the rows [grid, 1024) of a weight-gradient slab region; zero-filled again after the check
    hipError_t slab_rows(float* slabs, int grid, int row_len, const char* name) {
        const size_t lo = (size_t)grid * row_len, hi = (size_t)1024 * row_len;
        return grid < 1024 ? band((unsigned char*)(slabs + lo), (hi - lo) * 4, name, true) : hipSuccess;
    }
    hipError_t band(unsigned char* p, size_t bytes, const std::string& name, bool rezero) {
        bands.push_back(Band{name, p, bytes, rezero});
        return hipMemsetAsync(p, CANARY, bytes, st);
    }
    int check() {           // after the stream synchronisation
        std::vector<unsigned char> h;
        std::string bad;
        for (const Band& b : bands) {
            h.resize(b.bytes);
            HIPC(hipMemcpy(h.data(), b.p, b.bytes, hipMemcpyDeviceToHost));
            static const std::vector<unsigned char> want(1 << 20, (unsigned char)CANARY);
            for (size_t o = 0; o < b.bytes && bad.empty(); o += want.size()) {
                const size_t k = std::min(want.size(), b.bytes - o);
                if (memcmp(h.data() + o, want.data(), k) == 0) continue;
                size_t i = o;
                while (h[i] == (unsigned char)CANARY) ++i;
                bad = std::string(hook) + ": a kernel wrote past the end of " + b.name + " (guard byte " + std::to_string(i) + ")";
            }
            if (b.rezero) HIPC(hipMemsetAsync(b.p, 0, b.bytes, st));
        }
        bands.clear();
        HIPC(hipStreamSynchronize(st));
        return bad.empty() ? 0 : fail(-4, bad);
    }
};

// the end of an op-level call: launch errors, the stream wait, the canary bands
static int op_finish(mi_ctx* c, OpMem& m) {
    HIPC(hipGetLastError()); NETCHK(c);
    HIPC(hipStreamSynchronize(c->stream));
    return m.check();
}
// upload an activation tensor in the context's storage type
static int upload_act(mi_ctx* c, OpMem& m, const float* host, size_t n, void** dev) {
    HIPC(m.alloc(dev, n * 4));
    HIPC(hipStreamSynchronize(c->stream));          // (the fill runs on the context's stream, the copy on the null stream)
    if (c->bf) { auto h = host_to_bf16(host, n); HIPC(hipMemcpy(*dev, h.data(), n * 2, hipMemcpyHostToDevice)); }
    else HIPC(hipMemcpy(*dev, host, n * 4, hipMemcpyHostToDevice));
    return 0;
}
static int download_act(mi_ctx* c, const void* dev, float* host, size_t n) {
    if (c->bf) { std::vector<uint16_t> h(n); HIPC(hipMemcpy(h.data(), dev, n * 2, hipMemcpyDeviceToHost)); host_from_bf16(h.data(), host, n); }
    else HIPC(hipMemcpy(host, dev, n * 4, hipMemcpyDeviceToHost));
    return 0;
}
static int upload(OpMem& m, const void* host, size_t bytes, void** dev) {
    HIPC(m.alloc(dev, bytes));
    HIPC(hipStreamSynchronize(m.st));
    HIPC(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

int mi_op_conv3x3(mi_ctx* c, int32_t mode, int32_t cin, int32_t cout, int32_t hw, int32_t n, const void* in, int32_t in_is_u8,
                  int32_t relu_in, const float* w_ref, const float* bias, const float* res, const float* mask, const float* dout,
                  float* out, float* dbias_out) {
    ARG(c && w_ref && out && n >= 1, "null"); JOIN(c);
    ConvShape s;
    if (shape_of(cin, cout, hw, &s)) return -1;
    ARG((s == CS_3_16_64) == (in_is_u8 != 0) || mode == 1, "block1.conv takes uint8 frames");
    const std::string hook = "mi_op_conv3x3 mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    const size_t px = (size_t)n * hw * hw, es = c->bf ? 2 : 4;
    TensorDesc td{"w", 0, 0, (int64_t)cout * cin * 9, K_CONVW, cout, cin};
    std::vector<float> wdev(td.n);
    to_device_layout(td, w_ref, wdev.data());
    float *dw = nullptr, *db = nullptr;
    void *din = nullptr, *dres = nullptr, *dmask = nullptr, *ddout = nullptr, *dout_buf = nullptr;
    if (int r = upload(m, wdev.data(), td.n * 4, (void**)&dw)) return r;
    if (bias) { if (int r = upload(m, bias, cout * 4, (void**)&db)) return r; }
    const int out_ch = (mode == 1) ? cin : cout;
    if (mode != 1) {
        if (in_is_u8) { if (int r = upload(m, in, px * 3, &din)) return r; }
        else if (int r = upload_act(c, m, (const float*)in, px * cin, &din)) return r;
    }
    // the weight gradient: slabs [grid][td.n + cout] summed into g (the reduction adds: zero fill)
    auto wgrad_out = [&](float** g, int grid) -> int {
        HIPC(m.out(g, (td.n + cout) * 4, "the weight / bias gradient", 0));
        HIPC(m.slab_rows(c->slabs, grid, (int)td.n + cout, "the weight-gradient slab rows past the grid"));
        return 0;
    };
    auto read_wgrad = [&](const float* g) -> int {
        std::vector<float> hg(td.n + cout);
        HIPC(hipMemcpy(hg.data(), g, hg.size() * 4, hipMemcpyDeviceToHost));
        to_ref_layout(td, hg.data(), out);
        if (dbias_out) memcpy(dbias_out, hg.data() + td.n, cout * 4);
        return 0;
    };
    if (mode >= 3) {        // a block's first conv fused with the block's max pool (bf16): 3 = forward -> pooled map,
                            // 4 = weight gradient, 5 = data gradient -- both from the POOLED gradient + the forward's arg-max bytes
        ARG(c->bf && (s == CS_3_16_64 || s == CS_16_32_32 || s == CS_32_32_16), "fused conv+pool modes: block1/2/3.conv in bf16 precision only");
        ARG(mode <= 7 && !(mode >= 5 && s == CS_3_16_64) && in, "mode");
        ARG(mode == 3 || mode == 5 || c->slabs, "modes 4 / 6: weight gradients need an IMPALA context");
        ARG(mode < 6 || conv_bwd_fused_grid(s, n) > 0, "modes 6 / 7: block2.conv / block3.conv");
        ARG(mode == 3 || dout, "dout");
        const size_t pp = (size_t)n * (hw / 2) * (hw / 2) * cout;
        void *dp = nullptr, *dgi = nullptr; uint8_t* di = nullptr; unsigned short* dbank = nullptr; BankDesc* ddesc = nullptr;
        HIPC(m.out(&dp, pp * 2, "the pooled map")); HIPC(m.out(&di, pp, "the arg-max bytes", 0));
        ConvArgs a{};
        a.in = din; a.w = dw; a.bias = db; a.n = n; a.bf16 = 1; a.lut16 = c->lut16;
        if (s == CS_3_16_64) launch_conv1_pool_fwd_bf16(a, c->lut16, dp, di, c->stream);
        else {
            const long long bf_len = (long long)cout * bank_ws(cin), bd_len = (long long)cin * bank_ws(cout);
            BankDesc d[2] = {{0, 0, cout, cin, cout, cin, 0, bank_ws(cin), cin == 32 ? 9 : 5}, {0, bf_len, cin, cout, cout, cin, 1, bank_ws(cout), cout == 32 ? 9 : 5}};
            HIPC(m.alloc(&dbank, (size_t)(bf_len + bd_len) * 2));
            if (int r = upload(m, d, sizeof d, (void**)&ddesc)) return r;
            launch_pack_banks(dw, dbank, ddesc, 2, c->stream);
            a.wbank = dbank;
            ARG(launch_conv_pool_fwd_bf16(s, a, dp, di, c->stream), "no fused kernel");
        }
        HIPC(hipGetLastError()); NETCHK(c);
        HIPC(hipStreamSynchronize(c->stream));
        if (mode == 3) {
            if (int r = m.check()) return r;
            return download_act(c, dp, out, pp);
        }
        if (int r = upload_act(c, m, dout, pp, &ddout)) return r;
        if (mode == 4) {
            float* g = nullptr;
            const int grid = wgrad_grid_for(s, n, 1);
            if (int r = wgrad_out(&g, grid)) return r;
            WgradArgs wa{};
            wa.in = din; wa.dout = ddout; wa.partial = c->slabs; wa.n = n; wa.bf16 = 1; wa.lut16 = c->lut16; wa.pool_arg = di;
            launch_conv_wgrad(s, wa, c->stream);
            launch_reduce_slabs(c->slabs, grid, (int)td.n + cout, g, (int)td.n, g + td.n, cout, c->stream);
            if (int r = op_finish(c, m)) return r;
            return read_wgrad(g);
        }
        // 5: data gradient; 6 / 7: the fused data + weight gradient launch (block2.conv, block3.conv), returning dW (+ db) / dx
        HIPC(m.out(&dgi, px * cin * 2, "the data gradient"));
        ConvArgs g{};
        g.in = ddout; g.pool_arg = di; g.w = dw; g.out = dgi; g.n = n; g.bf16 = 1; g.wbank = dbank + (long long)cout * bank_ws(cin);
        float* gw = nullptr;
        const int fgrid = mode >= 6 ? conv_bwd_fused_grid(s, n) : 0;
        if (mode >= 6) { g.wg_in = din; g.wg_partial = c->slabs; if (int r = wgrad_out(&gw, fgrid)) return r; }
        launch_conv_dgrad(s, g, c->stream);
        if (mode >= 6) launch_reduce_slabs(c->slabs, fgrid, (int)td.n + cout, gw, (int)td.n, gw + td.n, cout, c->stream);
        if (int r = op_finish(c, m)) return r;
        return mode == 6 ? read_wgrad(gw) : download_act(c, dgi, out, px * cin);
    }
    if (mode >= 1) { ARG(dout, "dout"); if (int r = upload_act(c, m, dout, px * cout, &ddout)) return r; }
    if (res) { if (int r = upload_act(c, m, res, px * out_ch, &dres)) return r; }
    if (mask) { if (int r = upload_act(c, m, mask, px * out_ch, &dmask)) return r; }
    if (mode <= 1) {
        HIPC(m.out(&dout_buf, px * out_ch * es, mode == 0 ? "the conv output" : "the data gradient"));
        ConvArgs a{};
        a.in = (mode == 0) ? din : ddout; a.idx = nullptr; a.in_base = 0; a.w = dw; a.bias = (mode == 0) ? db : nullptr;
        a.res = dres; a.mask = dmask; a.out = dout_buf; a.lut = c->lut; a.n = n; a.relu_in = (mode == 0) ? relu_in : 0; a.bf16 = c->bf;
        a.lut16 = c->bf ? c->lut16 : nullptr;
        if (mode == 0) launch_conv_fwd(s, a, c->stream); else launch_conv_dgrad(s, a, c->stream);
        if (int r = op_finish(c, m)) return r;
        return download_act(c, dout_buf, out, px * out_ch);
    }
    ARG(c->slabs, "wgrad needs an IMPALA context");
    float* g = nullptr;
    const int grid = wgrad_grid_for(s, n, c->bf);
    if (int r = wgrad_out(&g, grid)) return r;
    WgradArgs a{};
    a.in = din; a.idx = nullptr; a.in_base = 0; a.dout = ddout; a.partial = c->slabs; a.lut = c->lut; a.n = n; a.relu_in = relu_in; a.bf16 = c->bf;
    a.lut16 = c->bf ? c->lut16 : nullptr;
    launch_conv_wgrad(s, a, c->stream);
    launch_reduce_slabs(c->slabs, grid, (int)td.n + cout, g, (int)td.n, g + td.n, cout, c->stream);
    if (int r = op_finish(c, m)) return r;
    return read_wgrad(g);
}

// Fused residual block of the bf16 mode, op level.  mode 0: (x, w1, b1, w2, b2) -> a = conv1(relu(x)) + b1, y = conv2(relu(a)) + b2 + x.
// mode 1: (dy = x, a_fwd, x_fwd, w1, w2) -> out_a = d a = convT2(dy) * (a_fwd > 0), out_y = d x = convT1(d a) * (x_fwd > 0) + dy.
// mode 4: res1 + res2 in one launch as net_forward runs them in training mode: w1 / b1 = res1's (conv1; conv2), w2 / b2 = res2's,
// out_a = (A1; A2), out_y = (P1; P2).
int mi_op_resblock(mi_ctx* c, int32_t mode, int32_t ch, int32_t hw, int32_t n, const float* x, const float* w1_ref, const float* b1,
                   const float* w2_ref, const float* b2, const float* a_fwd, const float* x_fwd, float* out_a, float* out_y) {
    ARG(c && x && w1_ref && w2_ref && out_a && out_y && n >= 1, "null"); JOIN(c);
    ARG(c->bf, "the fused residual-block kernels exist in bf16 precision only");
    ARG(mode >= 0 && mode <= 4, "mode");
    ARG((mode == 0 || mode >= 3) ? (b1 && b2) : (a_fwd && x_fwd), "modes 0 / 3 / 4 need the biases, modes 1 / 2 the forward tensors");
    ConvShape s;
    if (shape_of(ch, ch, hw, &s)) return -1;
    const std::string hook = "mi_op_resblock mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    const size_t X = (size_t)n * hw * hw * ch, wl = (size_t)ch * ch * 9;
    const int nc = mode == 4 ? 4 : 2;           // convs: (w1, w2), or mode 4's (res1.conv1, res1.conv2, res2.conv1, res2.conv2)
    const float* wsrc[4] = {w1_ref, w2_ref, nullptr, nullptr};
    const float* bsrc[4] = {b1, b2, nullptr, nullptr};
    if (mode == 4) { wsrc[1] = w1_ref + wl; wsrc[2] = w2_ref; wsrc[3] = w2_ref + wl; bsrc[1] = b1 + ch; bsrc[2] = b2; bsrc[3] = b2 + ch; }
    TensorDesc td{"w", 0, 0, (int64_t)wl, K_CONVW, ch, ch};
    std::vector<float> wdev((size_t)nc * (wl + ch), 0.f);
    for (int k = 0; k < nc; ++k) {
        to_device_layout(td, wsrc[k], wdev.data() + k * wl);
        if (bsrc[k]) memcpy(wdev.data() + nc * wl + k * ch, bsrc[k], ch * 4);
    }
    float* dparams = nullptr; unsigned short* dbanks = nullptr; BankDesc* ddesc = nullptr;
    void *dx = nullptr, *da = nullptr, *dxf = nullptr;
    if (int r = upload(m, wdev.data(), wdev.size() * 4, (void**)&dparams)) return r;
    const float* bias = dparams + nc * wl;
    const int ws = bank_ws(ch), nk = ch == 32 ? 9 : 5;
    const long long bl = (long long)ch * ws;
    // bank k feeds the kernel's k-th conv: forward the convs as stored; backward (w2^T, w1^T)
    const bool tr = (mode == 1 || mode == 2);
    BankDesc d[4];
    for (int k = 0; k < nc; ++k) d[k] = BankDesc{tr ? (k == 0 ? (long long)wl : 0) : (long long)(k * wl), k * bl, ch, ch, ch, ch, tr ? 1 : 0, ws, nk};
    HIPC(m.alloc(&dbanks, (size_t)nc * bl * 2));
    if (int r = upload(m, d, sizeof(BankDesc) * nc, (void**)&ddesc)) return r;
    launch_pack_banks(dparams, dbanks, ddesc, nc, c->stream);
    if (int r = upload_act(c, m, x, X, &dx)) return r;
    if (mode == 2) {        // whole backward of a 16-channel block: out_y = dx, out_a[0 .. 2*(9*ch*ch + ch)) = {dW1, db1, dW2, db2} (reference layout)
        ARG((s == CS_16_16_32 || s == CS_32_32_16 || s == CS_32_32_8) && c->slabs, "the whole-backward kernels exist for the 16-channel @32x32 and 32-channel @16x16 blocks (IMPALA context)");
        if (int r = upload_act(c, m, a_fwd, X, &da)) return r;
        if (int r = upload_act(c, m, x_fwd, X, &dxf)) return r;
        const int grid = s == CS_16_16_32 ? resblock_bwd_full_grid(n) : resblock_bwd_full32_grid(s, n), slab = (int)wl + ch;
        void* doy = nullptr; float* g = nullptr;
        HIPC(m.out(&doy, X * 2, "the data gradient"));
        HIPC(m.out(&g, (size_t)2 * slab * 4, "the weight / bias gradients", 0));
        float* sl2 = c->slabs; float* sl1 = c->slabs + (size_t)1024 * slab;
        HIPC(m.slab_rows(sl2, grid, slab, "conv2's weight-gradient slab rows past the grid"));
        HIPC(m.slab_rows(sl1, grid, slab, "conv1's weight-gradient slab rows past the grid"));
        if (s == CS_16_16_32) launch_resblock_bwd_full_bf16(dx, da, dxf, doy, nullptr, n, dbanks, dbanks + bl, sl2, sl1, c->stream);
        else launch_resblock_bwd_full32_bf16(s, dx, da, dxf, doy, nullptr, n, dbanks, dbanks + bl, sl2, sl1, c->stream);
        launch_reduce_slabs(sl1, grid, slab, g, (int)wl, g + wl, ch, c->stream);
        launch_reduce_slabs(sl2, grid, slab, g + slab, (int)wl, g + slab + wl, ch, c->stream);
        if (int r = op_finish(c, m)) return r;
        std::vector<float> hg(2 * slab);
        HIPC(hipMemcpy(hg.data(), g, hg.size() * 4, hipMemcpyDeviceToHost));
        to_ref_layout(td, hg.data(), out_a); memcpy(out_a + wl, hg.data() + wl, ch * 4);
        to_ref_layout(td, hg.data() + slab, out_a + slab); memcpy(out_a + slab + wl, hg.data() + slab + wl, ch * 4);
        return download_act(c, doy, out_y, X);
    }
    void* o[4] = {};        // mode 4: A1, P1, A2, P2; otherwise out_a, out_y
    static const char* oname[4] = {"A1 (res1.conv1 output)", "P1 (res1 output)", "A2 (res2.conv1 output)", "P2 (block output)"};
    for (int k = 0; k < (mode == 4 ? 4 : 2); ++k) HIPC(m.out(&o[k], X * 2, mode == 4 ? oname[k] : (k ? "out_y" : "out_a")));
    if (mode == 4) {
        const float* bb[4] = {bias, bias + ch, bias + 2 * ch, bias + 3 * ch};
        const unsigned short* bk[4] = {dbanks, dbanks + bl, dbanks + 2 * bl, dbanks + 3 * bl};
        launch_resblock_pair_bf16(s, dx, bb, o[0], o[1], o[2], o[3], n, bk, c->stream);
    } else if (mode == 3) {        // res1 + res2 in one launch, both with (w1, b1, w2, b2): out_a = second conv1 output, out_y = second block output
        const float* bb[4] = {bias, bias + ch, bias, bias + ch};
        const unsigned short* bk[4] = {dbanks, dbanks + bl, dbanks, dbanks + bl};
        launch_resblock_pair_bf16(s, dx, bb, nullptr, nullptr, o[0], o[1], n, bk, c->stream);
    } else if (mode == 0) {
        launch_resblock_bf16(s, dx, bias, bias + ch, o[0], o[1], n, dbanks, dbanks + bl, c->stream);
    } else {
        if (int r = upload_act(c, m, a_fwd, X, &da)) return r;
        if (int r = upload_act(c, m, x_fwd, X, &dxf)) return r;
        launch_resblock_bwd_bf16(s, dx, da, dxf, o[0], o[1], n, dbanks, dbanks + bl, c->stream);
    }
    if (int r = op_finish(c, m)) return r;
    if (mode == 4) {
        for (int k = 0; k < 4; ++k)
            if (int r = download_act(c, o[k], (k & 1 ? out_y : out_a) + (k >> 1) * X, X)) return r;
        return 0;
    }
    if (int r = download_act(c, o[0], out_a, X)) return r;
    return download_act(c, o[1], out_y, X);
}

// Philox4x32-10 known-answer hook: n x {c0,c1,c2,c3,k0,k1} in, n x 4 output words and the n uniforms the sampler would draw
// for (seed = k0 | k1 << 32, counter = c0 | c1 << 32) out.
int mi_debug_philox(mi_ctx* c, const uint32_t* ctr_key6, int32_t n, uint32_t* out4, float* u_out) {
    ARG(c && ctr_key6 && out4 && u_out, "null"); JOIN(c); ARG(n >= 1 && n <= (1 << 24), "n");
    uint32_t *din = nullptr, *dout = nullptr; float* du = nullptr;
    HIPC(hipMalloc((void**)&din, (size_t)n * 24)); HIPC(hipMalloc((void**)&dout, (size_t)n * 16)); HIPC(hipMalloc((void**)&du, (size_t)n * 4));
    HIPC(hipMemcpy(din, ctr_key6, (size_t)n * 24, hipMemcpyHostToDevice));
    launch_philox_debug(din, n, dout, du, c->stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(out4, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(u_out, du, (size_t)n * 4, hipMemcpyDeviceToHost));
    hipFree(din); hipFree(dout); hipFree(du);
    return 0;
}

// The fused GRU step of the pipelined rollout (gru_cell.hip gru_step_kernel) on caller data, for tests: n rows, width H (any multiple of 64 up
// to 512, independent of the context's), weights in nn.GRU's layout.  h_out = h' (and h_copy = the kernel's second copy of it, if not null).
int mi_debug_gru_step(mi_ctx* c, int32_t n, int32_t H, const float* x, const float* h, const float* done, const float* w_ih, const float* w_hh,
                      const float* b_ih, const float* b_hh, float* h_out, float* h_copy) {
    ARG(c && x && h && done && w_ih && w_hh && b_ih && b_hh && h_out, "null"); JOIN(c);
    ARG(n >= 1 && n <= 65536 && H >= 64 && H <= 512 && H % 64 == 0, "n in [1, 65536], H a multiple of 64 in [64, 512]");
    const size_t nh = (size_t)n * H, w = (size_t)3 * H * H;
    std::vector<float*> d(9, nullptr);
    const size_t sz[9] = {nh, nh, (size_t)n, w, w, (size_t)3 * H, (size_t)3 * H, nh, nh};
    const float* src[7] = {x, h, done, w_ih, w_hh, b_ih, b_hh};
    int rc = 0;
    for (int i = 0; i < 9 && !rc; ++i) if (hipMalloc((void**)&d[i], sz[i] * 4) != hipSuccess) rc = fail(-2, "hipMalloc failed");
    for (int i = 0; i < 7 && !rc; ++i) if (hipMemcpy(d[i], src[i], sz[i] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(-2, "upload failed");
    if (!rc) {
        launch_gru_step(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], n, H, c->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(-4, "gru_step_kernel failed");
    }
    if (!rc && hipMemcpy(h_out, d[7], nh * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-2, "download failed");
    if (!rc && h_copy && hipMemcpy(h_copy, d[8], nh * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-2, "download failed");
    for (float* p : d) if (p) hipFree(p);
    return rc;
}

// The GRU over a trajectory (gru_seq.hip) on caller data, for tests: n envs x T steps, rows time-major, width H (independent of the context's).
// Forward: out_h = h_t of all rows.  With dOut (dL/dh_t of all rows) also the backward pass through time and the GEMMs behind it, exactly as
// mi_minibatch_rec issues them: dX, dW_ih, dW_hh, db_ih, db_hh (from zero).
int mi_debug_gru_seq(mi_ctx* c, int32_t T, int32_t n, int32_t H, const float* x, const float* h0, const float* mask, const float* w_ih, const float* w_hh,
                     const float* b_ih, const float* b_hh, const float* dOut, float* out_h, float* dX, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh) {
    ARG(c && x && h0 && mask && w_ih && w_hh && b_ih && b_hh && out_h, "null"); JOIN(c);
    ARG(!dOut || (dX && dW_ih && dW_hh && db_ih && db_hh), "null gradient outputs");
    ARG(gru_seq_width_ok(H), "H must be a multiple of 64 in [64, 512]");
    ARG(T >= 1 && n >= 1 && (int64_t)T * n <= 65536, "T, n >= 1 and T * n <= 65536");
    const size_t N = (size_t)T * n, NH = N * H, W = (size_t)3 * H * H, B = (size_t)3 * H;
    enum { X = 0, H0, MK, WIH, WHH, BIH, BHH, DOUT, GI, OUT, SV, DGI, DGH, HM, DX, GWIH, GWHH, GBIH, GBHH, NBUF };
    const size_t sz[NBUF] = {NH, (size_t)n * H, N, W, W, B, B, NH, 3 * NH, NH, 4 * NH, 3 * NH, 3 * NH, NH, NH, W, W, B, B};
    const float* src[8] = {x, h0, mask, w_ih, w_hh, b_ih, b_hh, dOut};
    std::vector<float*> d(NBUF, nullptr);
    int rc = 0;
    for (int i = 0; i < NBUF && !rc; ++i) if (hipMalloc((void**)&d[i], sz[i] * 4) != hipSuccess) rc = fail(-2, "hipMalloc failed");
    for (int i = 0; i < 8 && !rc; ++i) if (src[i] && hipMemcpy(d[i], src[i], sz[i] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(-2, "upload failed");
    for (int i = GWIH; i < NBUF && !rc; ++i) if (hipMemset(d[i], 0, sz[i] * 4) != hipSuccess) rc = fail(-2, "hipMemset failed");
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(-2, "sync failed");
    if (!rc) {
        linear_fwd(c, d[X], 0, d[WIH], d[BIH], d[GI], (int)N, H, 3 * H, 0);
        launch_gru_seq_fwd(d[GI], d[H0], d[MK], d[WHH], d[BHH], d[OUT], d[SV], T, n, H, c->stream);
        if (dOut) {
            launch_gru_seq_bwd(d[DOUT], d[OUT], d[H0], d[MK], d[SV], d[WHH], d[DGI], d[DGH], d[HM], T, n, H, c->stream);
            linear_wgrad(c, d[DGI], d[X], 0, d[GWIH], d[GBIH], (int)N, H, 3 * H);
            linear_wgrad(c, d[DGH], d[HM], 0, d[GWHH], d[GBHH], (int)N, H, 3 * H);
            linear_dgrad(c, d[DGI], d[WIH], nullptr, d[DX], (int)N, H, 3 * H);
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(-4, "GRU sequence kernels failed");
        if (!rc) if (const char* lf = mi_launch_failed_take()) rc = fail(-4, lf);
    }
    auto down = [&](float* dst, int k) { if (!rc && hipMemcpy(dst, d[k], sz[k] * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-2, "download failed"); };
    down(out_h, OUT);
    if (dOut) { down(dX, DX); down(dW_ih, GWIH); down(dW_hh, GWHH); down(db_ih, GBIH); down(db_hh, GBHH); }
    for (float* p : d) if (p) hipFree(p);
    return rc;
}

// Measurement hook ("hipGraph"): wall-clock microseconds per policy step of slot t -- the step's launches (conv stack,
// embedder.fc, fused heads + sample: 5 kernels in bf16 mode) followed by a stream wait, `iters` times back to back -- issued eagerly
// (mode 0) or as ONE replay of a graph captured from the same launches (mode 1).  What a captured group step could save on the
// rollout's dependency chain, without touching the production path (whose per-step arguments change: slot, counters, ticket).
int mi_debug_step_latency(mi_ctx* c, int32_t t, int32_t iters, int32_t mode, float* us_out) {
    ARG(c && us_out, "null"); JOIN(c); ARG(t >= 0 && t <= c->T && iters >= 1 && (mode == 0 || mode == 1), "t / iters / mode");
    const int E = c->E;
    InputSrc src{obs_ring(c), nullptr, (long long)t * E};
    auto issue = [&]() {
        c->prof.phase = 0;
        net_forward(c, src, E, {.recurrent = true, .heads = false});
        launch_heads_sample(c->feat, c->params + c->wh_off, c->params + c->bh_off, E, c->H, c->A, nullptr, 1234ull, (unsigned long long)t * E,
                            nullptr, nullptr, c->value + (size_t)t * E, c->h_pack, nullptr, nullptr, nullptr, nullptr, c->stream, nullptr, nullptr, 0, c->lse);
    };
    const bool prof_on = c->prof.on; c->prof.on = false;       // (no event records inside a capture)
    issue();                                                   // warm: packed banks in place, lazy function attributes set
    HIPC(hipGetLastError()); NETCHK(c);
    HIPC(hipStreamSynchronize(c->stream));
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    if (mode == 1) {
        HIPC(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        issue();
        HIPC(hipStreamEndCapture(c->stream, &graph));
        HIPC(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        HIPC(hipGraphLaunch(exec, c->stream)); HIPC(hipStreamSynchronize(c->stream));
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < iters; ++k) {
        if (mode == 1) HIPC(hipGraphLaunch(exec, c->stream)); else issue();
        HIPC(hipStreamSynchronize(c->stream));
    }
    const auto t1 = std::chrono::steady_clock::now();
    *us_out = (float)(std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count() / 1e3 / iters);
    if (exec) hipGraphExecDestroy(exec);
    if (graph) hipGraphDestroy(graph);
    c->prof.on = prof_on;
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

// Measurement hook ("Lanes"): do the group streams of this context run side by side?  One 64-thread workgroup per
// stream in `mask` sleeps a fixed number of times -- no flag, no clock, no memory traffic, so it cannot wait on anything -- and the host
// times first launch to last completion: one lane's time when the lanes sit on hardware queues of their own, a multiple where they share.
__global__ void __launch_bounds__(64) lane_probe_kernel(int iters) {
    for (int i = 0; i < iters; ++i) __builtin_amdgcn_s_sleep(127);
}
int mi_debug_lane_probe(mi_ctx* c, int32_t mask, int32_t iters, float* usec) {
    ARG(c && usec, "null"); JOIN(c);
    ARG(mask > 0 && mask < (1 << c->n_groups) && iters >= 1, "mask (bits of this context's groups) / iters");
    for (int g = 0; g < c->n_groups; ++g) ARG(c->grp[g].stream && !c->grp[g].busy, "call mi_rollout_groups first; no group step in flight");
    if (iters > 4096) iters = 4096;
    for (int g = 0; g < c->n_groups; ++g) if (mask >> g & 1) HIPC(hipStreamSynchronize(c->grp[g].stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (int g = 0; g < c->n_groups; ++g) if (mask >> g & 1) lane_probe_kernel<<<1, 64, 0, c->grp[g].stream>>>(iters);
    for (int g = 0; g < c->n_groups; ++g) if (mask >> g & 1) HIPC(hipStreamSynchronize(c->grp[g].stream));
    const auto t1 = std::chrono::steady_clock::now();
    HIPC(hipGetLastError());
    *usec = (float)(std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count() / 1e3);
    return 0;
}

// Read back what the last training-mode pass (mi_minibatch) left in the activation buffers, as fp32 NHWC: which = 8 * block + k with
// k = 0 P0 (pooled map), 1 A1, 2 P1, 3 A2, 4 P2 (res1.conv1 out, res1 out, res2.conv1 out, block out), 5 the max-pool arg-max bytes
// (window position ky*3+kx as float); which = 100: the 256 features.  For teacher-forced backward parity tests.
int mi_debug_read(mi_ctx* c, int32_t which, int32_t n, float* out) {
    ARG(c && out, "null"); JOIN(c); ARG(n >= 1 && n <= c->NB, "n must be in [1, max_batch]");
    if (which == 100 || which == 101 || which == 102) {
        // after a recurrent pass (mi_minibatch_rec) the features -- the embedder output x -- sit in their own buffer: feat holds h_t (101), dfeat dX (102)
        ARG(which == 100 || c->rec_last, "which = 101 / 102: only after mi_minibatch_rec");
        const float* srcp = which == 102 ? c->dfeat : (which == 100 && c->rec_last) ? c->rec_x : c->feat;
        HIPC(hipMemcpyAsync(out, srcp, (size_t)n * c->H * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        return 0;
    }
    ARG(c->cfg.arch == MI_ARCH_IMPALA && which >= 0 && which < 24 && (which & 7) <= 5, "which");
    const Block& k = c->blk[which >> 3];
    const size_t pe = (size_t)n * (k.hin / 2) * (k.hin / 2) * k.cout;
    HIPC(hipStreamSynchronize(c->stream));
    if ((which & 7) == 5) {
        std::vector<uint8_t> h(pe);
        HIPC(hipMemcpy(h.data(), k.PI, pe, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < pe; ++i) out[i] = (float)h[i];
        return 0;
    }
    const float* src[5] = {k.P0, k.A1, k.P1, k.A2, k.P2};
    return download_act(c, src[which & 7], out, pe);
}

int mi_op_maxpool(mi_ctx* c, int32_t mode, int32_t n, int32_t hw, int32_t ch, const float* in, const float* dout, float* out) {
    ARG(c && in && out, "null"); JOIN(c); ARG(n >= 1, "n");
    ARG((hw == 64 && ch == 16) || (hw == 32 && ch == 32) || (hw == 16 && ch == 32), "max pool shapes of the IMPALA blocks only: (64,16), (32,32), (16,32)");
    ARG(mode == 0 || dout, "dout");
    OpMem m(mode == 0 ? "mi_op_maxpool mode 0" : "mi_op_maxpool mode 1", c->stream);
    const size_t X = (size_t)n * hw * hw * ch, p = X / 4, es = c->bf ? 2 : 4;
    void *din = nullptr, *dp = nullptr, *dd = nullptr, *dg = nullptr; uint8_t* di = nullptr;
    if (int r = upload_act(c, m, in, X, &din)) return r;
    HIPC(m.out(&dp, p * es, "the pooled map")); HIPC(m.out(&di, p, "the arg-max bytes", 0));
    if (c->bf) launch_maxpool_fwd_bf16(din, dp, di, n, hw, ch, c->stream); else launch_maxpool_fwd((const float*)din, (float*)dp, di, n, hw, ch, c->stream);
    if (mode != 0) {
        if (int r = upload_act(c, m, dout, p, &dd)) return r;
        HIPC(m.out(&dg, X * es, "the data gradient"));
        if (c->bf) launch_maxpool_bwd_bf16(dd, di, dg, n, hw, ch, c->stream); else launch_maxpool_bwd((const float*)dd, di, (float*)dg, n, hw, ch, c->stream);
    }
    if (int r = op_finish(c, m)) return r;
    return mode == 0 ? download_act(c, dp, out, p) : download_act(c, dg, out, X);
}

int mi_op_gemm(mi_ctx* c, int32_t M, int32_t N, int32_t K, const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk,
               int64_t sbn, float* C) {
    ARG(c && A && B && C, "null"); JOIN(c);
    const size_t na = (size_t)((M - 1) * sam + (K - 1) * sak + 1), nb = (size_t)((K - 1) * sbk + (N - 1) * sbn + 1);
    float *da = nullptr, *db = nullptr, *dc = nullptr;
    DevPool m(hip_pool());
    HIPC(m.dev(&da, na)); HIPC(m.dev(&db, nb)); HIPC(m.dev(&dc, (size_t)M * N));
    HIPC(hipMemcpy(da, A, na * 4, hipMemcpyHostToDevice)); HIPC(hipMemcpy(db, B, nb * 4, hipMemcpyHostToDevice));
    GemmArgs g{};
    g.ws = c->gemm_ws; g.ws_floats = c->gemm_ws_floats;
    g.A = da; g.B = db; g.C = dc; g.M = M; g.N = N; g.K = K; g.sam = sam; g.sak = sak; g.sbk = sbk; g.sbn = sbn; g.ldc = N;
    launch_gemm(g, c->stream);
    HIPC(hipGetLastError()); NETCHK(c);
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(C, dc, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// embedder.fc's bf16 matrix-core kernels (fc_bf16.hip) on caller data, through the production launchers with the arguments
// backward_impala_bf16 / forward_impala_bf16 pass; independent of the context's sizes and precision.  D = the width (a multiple of 64 in
// [64, 512]), n rows, K = 2048 inputs.  x goes up rounded to bf16 (host_to_bf16), W [D][2048] through launch_fc_pack.
// (Production fills fc_wp / fc_wt in the fc section of repack_all_kernel, conv_bf16.hip, not through launch_fc_pack: that the two write the
// same images is checked by the end-to-end fc tests only, not here.)
//   mode 0: out = y [n][D] = relu(relu(x) W^T + b), launch_fc_fwd_bf16           mode 1: the same through launch_fc_fwd_small_bf16
//   mode 2: out = dx [n][2048] = (dy W) * (x > 0), launch_fc_dgrad_bf16 (bf16, widened); x is the mask source and is required: without a
//           mask the launcher takes the tiled kernel, which needs D % 128 == 0
//   mode 3: out = gW [D][2048], out_b = gb [D], both in / out: += dy^T relu(x) (launch_fc_tn with the engine's 8 M-float workspace) and
//           += colsum(dy) (launch_colsum_acc)
int mi_op_fc_bf16(mi_ctx* c, int32_t mode, int32_t n, int32_t D, const float* x, const float* W, const float* b, const float* dy,
                  float* out, float* out_b) {
    ARG(c && out, "null"); JOIN(c);
    ARG(mode >= 0 && mode <= 3, "mode");
    ARG(D >= 64 && D <= 512 && D % 64 == 0, "D must be a multiple of 64 in [64, 512]");
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]");
    ARG(mode != 2 || x, "mode 2 needs the mask source x (the data gradient without a mask has no kernel for every width)");
    ARG(x && (mode == 3 || W) && (mode >= 2 || b) && (mode <= 1 || dy) && (mode != 3 || out_b), "null");
    const std::string hook = "mi_op_fc_bf16 mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    constexpr int K = 2048;
    const size_t nx = (size_t)n * K, nd = (size_t)n * D, nw = (size_t)D * K;
    void* dxb = nullptr; float *dw = nullptr, *db = nullptr, *ddy = nullptr; unsigned short *wp = nullptr, *wt = nullptr;
    { const auto h = host_to_bf16(x, nx); if (int r = upload(m, h.data(), nx * 2, &dxb)) return r; }
    if (mode != 3) {
        if (int r = upload(m, W, nw * 4, (void**)&dw)) return r;
        HIPC(m.alloc(&wp, nw * 2)); HIPC(m.alloc(&wt, nw * 2));
        launch_fc_pack(dw, wp, wt, D, K, c->stream);
    }
    if (mode <= 1) {
        float* y = nullptr;
        if (int r = upload(m, b, (size_t)D * 4, (void**)&db)) return r;
        HIPC(m.out(&y, nd * 4, "y"));
        if (mode == 0) launch_fc_fwd_bf16(dxb, wp, db, y, n, D, c->stream);
        else launch_fc_fwd_small_bf16(dxb, wp, db, y, n, D, c->stream);
        if (int r = op_finish(c, m)) return r;
        HIPC(hipMemcpy(out, y, nd * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    if (int r = upload(m, dy, nd * 4, (void**)&ddy)) return r;
    if (mode == 2) {
        void* dxo = nullptr;
        HIPC(m.out(&dxo, nx * 2, "dx"));
        launch_fc_dgrad_bf16(ddy, wt, dxb, dxo, n, D, c->stream);
        if (int r = op_finish(c, m)) return r;
        std::vector<uint16_t> h(nx);
        HIPC(hipMemcpy(h.data(), dxo, nx * 2, hipMemcpyDeviceToHost));
        host_from_bf16(h.data(), out, nx);
        return 0;
    }
    // the engine's workspaces (mi_create): 8 M floats of split slabs, 64 x 4096 floats of column-sum partials.  Poisoned: the sums read
    // exactly what the kernels before them must have written
    const size_t ws_floats = (size_t)8 << 20;
    float *gw = nullptr, *gb = nullptr, *ws = nullptr, *col_ws = nullptr;
    HIPC(m.out(&gw, nw * 4, "gW")); HIPC(m.out(&gb, (size_t)D * 4, "gb"));
    HIPC(m.out(&ws, ws_floats * 4, "the split workspace")); HIPC(m.out(&col_ws, (size_t)64 * 4096 * 4, "the column-sum workspace"));
    HIPC(hipStreamSynchronize(c->stream));          // (the fills run on the context's stream, the copies on the null stream)
    HIPC(hipMemcpy(gw, out, nw * 4, hipMemcpyHostToDevice)); HIPC(hipMemcpy(gb, out_b, (size_t)D * 4, hipMemcpyHostToDevice));
    launch_fc_tn(ddy, (const unsigned short*)dxb, gw, ws, ws_floats, D, K, n, c->stream);
    launch_colsum_acc(ddy, n, D, D, gb, col_ws, c->stream);
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(out, gw, nw * 4, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(out_b, gb, (size_t)D * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The generic GEMM (gemm.hip: gemm_kernel, gemm_splitk_reduce) on caller data through the production launchers; independent of the
// context's sizes and precision.  d0, d1, d2 = (n, in, out) for forms 0 .. 2 and (M, N, K) for form 3.
//   form 0: linear_fwd    A = X [n][in], B = W [out][in], bias [out] or null -> C = Y [n][out]       flags: RELU_X, RELU_OUT, X_BF16
//   form 1: linear_dgrad  A = dY [n][out], B = W [out][in], mask [n][in] or null -> C = dX [n][in]   flags: X_BF16 (mask up as bf16, dX back widened)
//   form 2: linear_wgrad  A = dY [n][out], B = X [n][in]; C = gW [out][in] and gb [out] in / out     flags: RELU_X, X_BF16
//   form 3: launch_gemm itself with strides5 = {sam, sak, sbk, sbn, ldc}: A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn], C and mask
//           [M][ldc], bias [N] or null.  flags: RELU_OUT, ACCUMULATE (C in / out: its [M][N] part goes up), USE_WS (else a null workspace:
//           never split).  ws_floats < 0: the context's own; otherwise an override no larger than it.  Columns N .. ldc - 1 of C must
//           come back as poison: a write there fails with -4.
// plan2 = {split, k_chunk} of gemm_plan for the call.  The slabs of a split call are poisoned as well: the reduce reads what the GEMM wrote.
int mi_op_linear(mi_ctx* c, int32_t form, int32_t d0, int32_t d1, int32_t d2, const int64_t* strides5, int32_t flags, int64_t ws_floats,
                 const float* A, const float* B, const float* bias, const float* mask, float* C, float* gb, int32_t* plan2) {
    ARG(c && A && B && C && plan2, "null"); JOIN(c);
    ARG(form >= 0 && form <= 3, "form");
    ARG(d0 >= 1 && d1 >= 1 && d2 >= 1, "sizes must be positive");
    constexpr int64_t LIM = (int64_t)1 << 26;
    ARG(d0 <= 65536 && d1 <= 65536 && d2 <= 65536 && (int64_t)d0 * d1 <= LIM && (int64_t)d1 * d2 <= LIM && (int64_t)d0 * d2 <= LIM,
        "sizes: each at most 65536, every tensor at most 2^26 elements (the limit only keeps the hook's allocations sane)");
    static const int allowed[4] = {MI_LIN_RELU_X | MI_LIN_RELU_OUT | MI_LIN_X_BF16, MI_LIN_X_BF16, MI_LIN_RELU_X | MI_LIN_X_BF16,
                                   MI_LIN_RELU_OUT | MI_LIN_ACCUMULATE | MI_LIN_USE_WS};
    ARG(!(flags & ~allowed[form]), "flags: an option this form does not have");
    ARG(form == 3 || (!strides5 && ws_floats < 0), "strides5 and ws_floats belong to form 3");
    ARG(form != 0 || !mask, "form 0 has no mask");
    ARG(form != 1 || !bias, "form 1 has no bias");
    ARG(form != 2 || (gb && !bias && !mask && d2 <= COLSUM_MAX_N), "form 2: gb, no bias, no mask, out <= 4096");
    const bool bf = flags & MI_LIN_X_BF16, relu_x = flags & MI_LIN_RELU_X, relu_out = flags & MI_LIN_RELU_OUT;
    const std::string hook = "mi_op_linear form " + std::to_string(form);
    OpMem m(hook.c_str(), c->stream);
    auto up = [&](const float* h, size_t cnt, bool as_bf16, void** d) -> int {
        if (as_bf16) { const auto v = host_to_bf16(h, cnt); return upload(m, v.data(), cnt * 2, d); }
        return upload(m, h, cnt * 4, d);
    };
    GemmArgs g{};          // forms 0 .. 2: the sizes and the workspace linear_* will pass, for the plan alone
    g.ws = c->gemm_ws; g.ws_floats = c->gemm_ws_floats;
    void *dA = nullptr, *dB = nullptr, *dbias = nullptr, *dmask = nullptr;
    auto poison_slabs = [&](const GemmPlan& p) -> int {
        plan2[0] = p.split; plan2[1] = p.k_chunk;
        if (p.split > 1) HIPC(hipMemsetAsync(g.ws, 0xFF, (size_t)p.split * g.M * g.N * 4, c->stream));
        return 0;
    };
    if (form != 3) {
        const int n = d0, in = d1, out = d2;
        const size_t nx = (size_t)n * in, ny = (size_t)n * out, nw = (size_t)out * in;
        if (form == 0) { g.M = n; g.N = out; g.K = in; } else if (form == 1) { g.M = n; g.N = in; g.K = out; } else { g.M = out; g.N = in; g.K = n; }
        if (int r = poison_slabs(gemm_plan(g))) return r;
        if (form == 0) {
            float* y = nullptr;
            if (int r = up(A, nx, bf, &dA)) return r;
            if (int r = upload(m, B, nw * 4, &dB)) return r;
            if (bias) { if (int r = upload(m, bias, (size_t)out * 4, &dbias)) return r; }
            HIPC(m.out(&y, ny * 4, "Y"));
            linear_fwd(c, (const float*)dA, relu_x, (const float*)dB, (const float*)dbias, y, n, in, out, relu_out, bf);
            if (int r = op_finish(c, m)) return r;
            HIPC(hipMemcpy(C, y, ny * 4, hipMemcpyDeviceToHost));
            return 0;
        }
        if (form == 1) {
            void* dx = nullptr;
            if (int r = upload(m, A, ny * 4, &dA)) return r;
            if (int r = upload(m, B, nw * 4, &dB)) return r;
            if (mask) { if (int r = up(mask, nx, bf, &dmask)) return r; }
            HIPC(m.out(&dx, nx * (bf ? 2 : 4), "dX"));
            linear_dgrad(c, (const float*)dA, (const float*)dB, (const float*)dmask, (float*)dx, n, in, out, bf);
            if (int r = op_finish(c, m)) return r;
            if (!bf) { HIPC(hipMemcpy(C, dx, nx * 4, hipMemcpyDeviceToHost)); return 0; }
            std::vector<uint16_t> h(nx);
            HIPC(hipMemcpy(h.data(), dx, nx * 2, hipMemcpyDeviceToHost));
            host_from_bf16(h.data(), C, nx);
            return 0;
        }
        float *gw = nullptr, *dgb = nullptr;
        if (int r = upload(m, A, ny * 4, &dA)) return r;
        if (int r = up(B, nx, bf, &dB)) return r;
        HIPC(m.out(&gw, nw * 4, "gW")); HIPC(m.out(&dgb, (size_t)out * 4, "gb"));
        HIPC(hipStreamSynchronize(c->stream));          // (the fills run on the context's stream, the copies on the null stream)
        HIPC(hipMemcpy(gw, C, nw * 4, hipMemcpyHostToDevice)); HIPC(hipMemcpy(dgb, gb, (size_t)out * 4, hipMemcpyHostToDevice));
        linear_wgrad(c, (const float*)dA, (const float*)dB, relu_x, gw, dgb, n, in, out, bf);
        if (int r = op_finish(c, m)) return r;
        HIPC(hipMemcpy(C, gw, nw * 4, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(gb, dgb, (size_t)out * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    ARG(strides5, "form 3 needs strides5");
    const int M = d0, N = d1, K = d2;
    const int64_t sam = strides5[0], sak = strides5[1], sbk = strides5[2], sbn = strides5[3], ldc = strides5[4];
    ARG(sam >= 1 && sak >= 1 && sbk >= 1 && sbn >= 1 && ldc >= N, "form 3: positive strides, ldc >= N");
    ARG(sam <= LIM && sak <= LIM && sbk <= LIM && sbn <= LIM && ldc <= LIM, "form 3: a stride above 2^26");
    const int64_t na = (M - 1) * sam + (K - 1) * sak + 1, nb = (K - 1) * sbk + (N - 1) * sbn + 1, nc = (int64_t)M * ldc;
    ARG(na <= LIM && nb <= LIM && nc <= LIM, "form 3: an operand spans more than 2^26 elements");
    ARG(ws_floats < 0 || (size_t)ws_floats <= c->gemm_ws_floats, "ws_floats above the context's workspace");
    float* dc = nullptr;
    if (int r = upload(m, A, (size_t)na * 4, &dA)) return r;
    if (int r = upload(m, B, (size_t)nb * 4, &dB)) return r;
    if (bias) { if (int r = upload(m, bias, (size_t)N * 4, &dbias)) return r; }
    if (mask) { if (int r = upload(m, mask, (size_t)nc * 4, &dmask)) return r; }
    HIPC(m.out(&dc, (size_t)nc * 4, "C"));
    if (flags & MI_LIN_ACCUMULATE) {
        HIPC(hipStreamSynchronize(c->stream));          // (the fill runs on the context's stream, the copy on the null stream)
        HIPC(hipMemcpy2D(dc, (size_t)ldc * 4, C, (size_t)ldc * 4, (size_t)N * 4, M, hipMemcpyHostToDevice));
    }
    g.ws = (flags & MI_LIN_USE_WS) ? c->gemm_ws : nullptr;
    g.ws_floats = !g.ws ? 0 : ws_floats < 0 ? c->gemm_ws_floats : (size_t)ws_floats;
    g.A = (const float*)dA; g.B = (const float*)dB; g.C = dc; g.M = M; g.N = N; g.K = K;
    g.sam = sam; g.sak = sak; g.sbk = sbk; g.sbn = sbn; g.ldc = ldc;
    g.bias = (const float*)dbias; g.mask = (const float*)dmask; g.relu_out = relu_out; g.accumulate = (flags & MI_LIN_ACCUMULATE) ? 1 : 0;
    if (int r = poison_slabs(gemm_plan(g))) return r;
    launch_gemm(g, c->stream);
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(C, dc, (size_t)nc * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r)
        for (int64_t q = N; q < ldc; ++q) {
            uint32_t u; memcpy(&u, C + (size_t)r * ldc + q, 4);
            if (u != 0xFFFFFFFFu) return fail(-4, hook + ": a kernel wrote into the padding of C (row " + std::to_string(r) + ", column " + std::to_string(q) + ")");
        }
    return 0;
}

// The fixed-order sums of reduce.hip on caller data through the production launchers; independent of the context's sizes.  Every
// accumulation target is an OpMem::out buffer that starts from the caller's values, so an element written past its end trips a band.
//   mode 0: launch_reduce_slabs(src [a = nslab][b = slab_len], dst_w [n_w], dst_b [n_b] or null with n_b = 0)
//   mode 1: launch_reduce_all_slabs over n_desc layers, desc = n_desc x {src_off, w_off, b_off, nslab, slab_len, n_w} (SlabDesc's fields as
//           int64), src = the slab workspace of src_len floats, dst_w = one flat gradient vector of n_w floats
//   mode 2: launch_colsum_acc(src = dY [a = M][ld], N = b, dst_w = db [N]) with a workspace of exactly the engine's 64 x 4096 floats,
//           poisoned; the launcher refuses N > 4096 and then nothing is launched
int mi_op_reduce(mi_ctx* c, int32_t mode, const float* src, int64_t src_len, int32_t a, int32_t b, int32_t ld, const int64_t* desc, int32_t n_desc,
                 float* dst_w, int64_t n_w, float* dst_b, int32_t n_b) {
    ARG(c && src && dst_w, "null"); JOIN(c);
    ARG(mode >= 0 && mode <= 2, "mode");
    ARG(src_len >= 1 && src_len <= ((int64_t)1 << 28) && n_w >= 1 && n_w <= ((int64_t)1 << 28), "src_len and n_w must be in [1, 2^28]");
    const std::string hook = "mi_op_reduce mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    float *dsrc = nullptr, *dw = nullptr, *db = nullptr;
    if (mode == 0) {
        ARG(a >= 1 && b >= 1 && (int64_t)a * b == src_len, "mode 0: src is [nslab][slab_len]");
        ARG(n_b >= 0 && n_w + n_b <= b && (n_b == 0) == (dst_b == nullptr), "mode 0: n_w + n_b <= slab_len; dst_b null exactly when n_b == 0");
    } else if (mode == 1) {
        ARG(desc && n_desc >= 1 && n_desc <= 64, "mode 1: 1 to 64 layers");
        for (int k = 0; k < n_desc; ++k) {
            const int64_t* d = desc + 6 * k;
            ARG(d[3] >= 1 && d[3] <= (1 << 20) && d[4] >= 4 && d[4] <= (1 << 24) && d[5] >= 0 && d[5] <= d[4], "mode 1: nslab / slab_len / n_w");
            ARG(!(d[0] & 3) && !(d[1] & 3) && !(d[2] & 3) && !(d[4] & 3) && !(d[5] & 3), "mode 1: offsets, slab_len and n_w must be multiples of 4");
            ARG(d[0] >= 0 && d[0] + d[3] * d[4] <= src_len, "mode 1: a layer's slabs end past src");
            ARG(d[1] >= 0 && d[1] + d[5] <= n_w && d[2] >= 0 && d[2] + (d[4] - d[5]) <= n_w, "mode 1: a layer's gradients end past the flat vector");
        }
    } else {
        ARG(a >= 1 && b >= 1 && ld >= b && (int64_t)a * ld == src_len && n_w == b, "mode 2: src is [M][ld] with ld >= N, dst_w is [N]");
    }
    if (int r = upload(m, src, (size_t)src_len * 4, (void**)&dsrc)) return r;
    HIPC(m.out(&dw, (size_t)n_w * 4, mode == 1 ? "the flat gradient vector" : mode == 0 ? "dst_w" : "db"));
    if (dst_b) HIPC(m.out(&db, (size_t)n_b * 4, "dst_b"));
    HIPC(hipStreamSynchronize(c->stream));          // (the fills run on the context's stream, the copies on the null stream)
    HIPC(hipMemcpy(dw, dst_w, (size_t)n_w * 4, hipMemcpyHostToDevice));
    if (dst_b) HIPC(hipMemcpy(db, dst_b, (size_t)n_b * 4, hipMemcpyHostToDevice));
    if (mode == 0) {
        launch_reduce_slabs(dsrc, a, b, dw, (int)n_w, db, n_b, c->stream);
    } else if (mode == 1) {
        std::vector<SlabDesc> h(n_desc);
        int max_len = 0;
        for (int k = 0; k < n_desc; ++k) {
            const int64_t* d = desc + 6 * k;
            h[k] = SlabDesc{(long long)d[0], (long long)d[1], (long long)d[2], (int)d[3], (int)d[4], (int)d[5]};
            max_len = std::max(max_len, (int)d[4]);
        }
        SlabDesc* dd = nullptr;
        if (int r = upload(m, h.data(), sizeof(SlabDesc) * n_desc, (void**)&dd)) return r;
        launch_reduce_all_slabs(dsrc, dw, dd, n_desc, max_len, c->stream);
    } else {
        float* col_ws = nullptr;
        HIPC(m.out(&col_ws, (size_t)64 * COLSUM_MAX_N * 4, "the column-sum workspace"));
        launch_colsum_acc(dsrc, a, b, ld, dw, col_ws, c->stream);
    }
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(dst_w, dw, (size_t)n_w * 4, hipMemcpyDeviceToHost));
    if (dst_b) HIPC(hipMemcpy(dst_b, db, (size_t)n_b * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The optimizer tail on caller vectors, as mi_optimizer_step / mi_sae_optimizer_step launch it: the partial sums of squares, then Adam
// with the host scalars of adam_scalars.  p, g, m, v [n] are in / out; *gnorm_out = the unclipped norm.
//   variant 0: one vector, 128 partial sums (the plain PPO path)
//   variant 1: a second vector p2, g2, m2, v2 [n2] shares the norm -- 256 partial sums -- and takes Adam in four pieces
//              [off[k], off[k + 1]) with 0 = off[0] < .. < off[4] = n2: the gru_train branch of mi_optimizer_step
//   variant 2: sae_adam_kernel (torch's own constants) on one vector
int mi_op_adam(mi_ctx* c, int32_t variant, int64_t n, float* p, float* g, float* mm, float* v, int64_t n2, float* p2, float* g2, float* m2,
               float* v2, const int64_t* off5, float lr, float max_norm, int32_t step, float* gnorm_out) {
    ARG(c && p && g && mm && v && gnorm_out, "null"); JOIN(c);
    ARG(variant >= 0 && variant <= 2, "variant");
    ARG(n >= 1 && n <= ((int64_t)1 << 28) && step >= 1, "n must be in [1, 2^28], step is 1-based");
    const bool two = variant == 1;
    if (two) {
        ARG(p2 && g2 && m2 && v2 && off5 && n2 >= 4 && n2 <= ((int64_t)1 << 28), "variant 1: the second vector (n2 in [4, 2^28]) and its five offsets");
        ARG(off5[0] == 0 && off5[4] == n2 && off5[0] < off5[1] && off5[1] < off5[2] && off5[2] < off5[3] && off5[3] < off5[4], "variant 1: 0 = off[0] < .. < off[4] = n2");
    }
    const std::string hook = "mi_op_adam variant " + std::to_string(variant);
    OpMem m(hook.c_str(), c->stream);
    static const char* names[8] = {"p", "g", "m", "v", "p2", "g2", "m2", "v2"};
    float* host[8] = {p, g, mm, v, p2, g2, m2, v2};
    float* d[8] = {};
    const int nv = two ? 8 : 4;
    for (int k = 0; k < nv; ++k) HIPC(m.out(&d[k], (size_t)(k < 4 ? n : n2) * 4, names[k]));
    double* part = nullptr; float* gn = nullptr;
    HIPC(m.out(&part, (size_t)(two ? 256 : 128) * 8, "the partial sums of squares")); HIPC(m.out(&gn, 4, "the norm"));
    HIPC(hipStreamSynchronize(c->stream));          // (the fills run on the context's stream, the copies on the null stream)
    for (int k = 0; k < nv; ++k) HIPC(hipMemcpy(d[k], host[k], (size_t)(k < 4 ? n : n2) * 4, hipMemcpyHostToDevice));
    const AdamScalars a = adam_scalars(lr, step);
    launch_sumsq_partials(d[1], n, part, c->stream);
    if (variant == 2) {
        launch_sae_adam(d[0], d[1], d[2], d[3], n, part, max_norm, a.w1, a.beta2, a.w2, a.eps, a.step_size, a.bc2_sqrt, gn, c->stream);
    } else if (!two) {
        launch_adam(d[0], d[1], d[2], d[3], n, part, 128, max_norm, lr, a.beta1, a.beta2, a.eps, a.step_size, a.bc2_sqrt, gn, c->stream);
    } else {
        launch_sumsq_partials(d[5], n2, part + 128, c->stream);
        launch_adam(d[0], d[1], d[2], d[3], n, part, 256, max_norm, lr, a.beta1, a.beta2, a.eps, a.step_size, a.bc2_sqrt, gn, c->stream);
        for (int k = 0; k < 4; ++k)
            launch_adam(d[4] + off5[k], d[5] + off5[k], d[6] + off5[k], d[7] + off5[k], (long long)(off5[k + 1] - off5[k]), part, 256, max_norm, lr, a.beta1,
                        a.beta2, a.eps, a.step_size, a.bc2_sqrt, nullptr, c->stream);
    }
    if (int r = op_finish(c, m)) return r;
    for (int k = 0; k < nv; ++k) HIPC(hipMemcpy(host[k], d[k], (size_t)(k < 4 ? n : n2) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(gnorm_out, gn, 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_advnorm_merge on R caller triples {count, mean, M2} -> the merged triple
int mi_op_adv_merge(mi_ctx* c, const double* all, int32_t R, double* stats3_out) {
    ARG(c && all && stats3_out, "null"); JOIN(c); ARG(R >= 1 && R <= 4096, "R must be in [1, 4096]");
    OpMem m("mi_op_adv_merge", c->stream);
    double *dall = nullptr, *ds = nullptr;
    if (int r = upload(m, all, (size_t)R * 24, (void**)&dall)) return r;
    HIPC(m.out(&ds, 24, "the merged statistics"));
    launch_advnorm_merge(dall, R, ds, c->stream);
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(stats3_out, ds, 24, hipMemcpyDeviceToHost));
    return 0;
}

// The IPL kernels alone (ipl.hip) on caller arrays: what mi_ipl_minibatch launches between its network passes
int mi_op_ipl_loss(mi_ctx* c, int32_t n, int32_t A, const float* hout, const float* nv_raw, const int32_t* act, const float* rew,
                   const float* done, const mi_ipl_hparams* hp, float* rec8_out, float* dY_out, float* gnext_out, float* pred_out) {
    ARG(c && hout && nv_raw && act && rew && done && hp, "null"); JOIN(c);
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]"); ARG(A >= 1 && A <= 16, "A must be in [1, 16]");
    for (int k = 0; k < n; ++k) ARG(act[k] >= 0 && act[k] < A, "action out of range");
    OpMem m("mi_op_ipl_loss", c->stream);
    const size_t nh = (size_t)n * (A + 1);
    float *dh = nullptr, *dnvr = nullptr, *drew = nullptr, *ddone = nullptr; int32_t* dact = nullptr;
    if (int r = upload(m, hout, nh * 4, (void**)&dh)) return r;
    if (int r = upload(m, nv_raw, (size_t)n * 4, (void**)&dnvr)) return r;
    if (int r = upload(m, act, (size_t)n * 4, (void**)&dact)) return r;
    if (int r = upload(m, rew, (size_t)n * 4, (void**)&drew)) return r;
    if (int r = upload(m, done, (size_t)n * 4, (void**)&ddone)) return r;
    IplArgs a{};
    float *rec = nullptr, *seed = nullptr;
    HIPC(m.out(&a.nv, (size_t)n * 4, "nv")); HIPC(m.out(&a.dY, nh * 4, "dY")); HIPC(m.out(&a.g_next, (size_t)n * 4, "g_next"));
    HIPC(m.out(&a.pred, (size_t)n * 4, "pred")); HIPC(m.out(&a.rew_out, (size_t)n * 4, "rew_out"));
    HIPC(m.out(&a.partial, (size_t)ipl_blocks(n) * ipl_partial_cols(A) * 8, "the block partials"));
    HIPC(m.out(&rec, 8 * 4, "the record")); HIPC(m.out(&seed, nh * 4, "the next-side seed"));
    a.hout = dh; a.idx = nullptr; a.act = dact; a.rew = drew; a.done = ddone; a.n = n; a.A = A; a.inv_n_global = 1.0f / (float)n;
    a.gamma = hp->gamma; a.alpha = hp->alpha; a.entropy_coef = hp->entropy_coef;
    a.entropy_modified = (hp->flags & MI_IPL_ENTROPY_MODIFIED) != 0; a.reward_incentive = (hp->flags & MI_IPL_REWARD_INCENTIVE) != 0;
    a.adv_incentive = (hp->flags & MI_IPL_ADV_INCENTIVE) != 0; a.zero_obs_seed = (hp->flags & MI_IPL_DEBUG_ZERO_OBS_SEED) != 0;
    launch_ipl_next_value(a, dnvr, 1, 0, c->stream);
    launch_ipl_loss(a, rec, c->stream);
    launch_ipl_next_seed(a.g_next, seed, n, A, c->stream);
    if (int r = op_finish(c, m)) return r;
    if (rec8_out) HIPC(hipMemcpy(rec8_out, rec, 8 * 4, hipMemcpyDeviceToHost));
    if (dY_out) HIPC(hipMemcpy(dY_out, a.dY, nh * 4, hipMemcpyDeviceToHost));
    if (gnext_out) {        // read from the seed's value column: what the second backward pass receives; its logit columns must be zeros
        std::vector<float> h(nh);
        HIPC(hipMemcpy(h.data(), seed, nh * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < A; ++k) if (h[(size_t)i * (A + 1) + k] != 0.f) return fail(-4, "mi_op_ipl_loss: the next-side seed has a non-zero logit column");
            gnext_out[i] = h[(size_t)i * (A + 1) + A];
        }
    }
    if (pred_out) HIPC(hipMemcpy(pred_out, a.pred, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}
int mi_op_ipl_greedy(mi_ctx* c, int32_t n, int32_t A, const float* hout, int32_t* act_out) {
    ARG(c && hout && act_out, "null"); JOIN(c);
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]"); ARG(A >= 1 && A <= 16, "A must be in [1, 16]");
    OpMem m("mi_op_ipl_greedy", c->stream);
    float *dh = nullptr, *lp = nullptr, *v = nullptr; int32_t* da = nullptr;
    if (int r = upload(m, hout, (size_t)n * (A + 1) * 4, (void**)&dh)) return r;
    HIPC(m.out(&da, (size_t)n * 4, "act")); HIPC(m.out(&lp, (size_t)n * 4, "logp")); HIPC(m.out(&v, (size_t)n * 4, "value"));
    launch_ipl_greedy(dh, n, A, da, lp, v, c->stream);
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(act_out, da, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The distillation loss kernels alone (distill.hip) on caller arrays: what mi_distill_minibatch launches between its network passes.
// hout [n][A+1], target [n][A] (row s belongs to sample s); the mean runs over n_global * A elements.
int mi_op_distill_loss(mi_ctx* c, int32_t n, int32_t A, const float* hout, const float* target, int32_t n_global, float* rec8_out, float* dY_out) {
    ARG(c && hout && target, "null"); JOIN(c);
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]"); ARG(A >= 1 && A <= 16, "A must be in [1, 16]"); ARG(n_global >= 1, "n_global must be at least 1");
    OpMem m("mi_op_distill_loss", c->stream);
    const size_t nh = (size_t)n * (A + 1);
    float *dh = nullptr, *dt = nullptr, *rec = nullptr;
    if (int r = upload(m, hout, nh * 4, (void**)&dh)) return r;
    if (int r = upload(m, target, (size_t)n * A * 4, (void**)&dt)) return r;
    DistillArgs a{};
    HIPC(m.out(&a.dY, nh * 4, "dY")); HIPC(m.out(&a.partial, (size_t)distill_blocks(n) * 8, "the block partials")); HIPC(m.out(&rec, 8 * 4, "the record"));
    const double inv_count = 1.0 / ((double)n_global * A);
    a.hout = dh; a.idx = nullptr; a.target = dt; a.n = n; a.A = A; a.scale = (float)inv_count;
    launch_distill_loss(a, inv_count, rec, nullptr, 0, c->stream);
    if (int r = op_finish(c, m)) return r;
    if (rec8_out) HIPC(hipMemcpy(rec8_out, rec, 8 * 4, hipMemcpyDeviceToHost));
    if (dY_out) HIPC(hipMemcpy(dY_out, a.dY, nh * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The policy / value heads at update size (heads.hip) on caller data through the production launchers; independent of the context's sizes.
//   mode 0: launch_heads_fwd: out = hout [n][O] = feat [n][256] Wh^T + bh.  H must be 256.
//   mode 1: launch_heads_bwd with its slab sum: out = dfeat [n][H] = (dY [n][O] Wh) * (feat > 0 if relu_mask); gW [O][H] and gb [O] are in / out
//           (+= dY^T feat, += colsum(dY)).  The workspace is exactly the 512 * (O*H + O) floats the launcher asks for, poisoned: the slab
//           sum reads what the kernel must have written.  H <= 256.
// O <= 16 in both modes; what the kernels do not support is refused before anything is launched.
int mi_op_heads(mi_ctx* c, int32_t mode, int32_t n, int32_t H, int32_t O, const float* feat, const float* Wh, const float* bh, const float* dY,
                int32_t relu_mask, float* out, float* gW, float* gb) {
    ARG(c && feat && Wh && out, "null"); JOIN(c);
    ARG(mode == 0 || mode == 1, "mode");
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]");
    ARG(O >= 1 && O <= 16, "the heads kernels take at most 16 outputs (O in [1, 16])");
    ARG(mode == 0 ? H == 256 : (H >= 1 && H <= 256), "mode 0 (heads_fwd_kernel) needs H == 256, mode 1 (heads_bwd_kernel) H in [1, 256]");
    ARG(mode == 0 ? bh != nullptr : (dY && gW && gb), "mode 0 needs bh; mode 1 needs dY, gW and gb");
    const std::string hook = "mi_op_heads mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    const size_t nf = (size_t)n * H, nw = (size_t)O * H, ny = (size_t)n * O;
    float *dfe = nullptr, *dw = nullptr, *db = nullptr, *ddy = nullptr, *dout = nullptr;
    if (int r = upload(m, feat, nf * 4, (void**)&dfe)) return r;
    if (int r = upload(m, Wh, nw * 4, (void**)&dw)) return r;
    if (mode == 0) {
        if (int r = upload(m, bh, (size_t)O * 4, (void**)&db)) return r;
        HIPC(m.out(&dout, ny * 4, "hout"));
        launch_heads_fwd(dfe, dw, db, dout, n, O, c->stream);
        if (int r = op_finish(c, m)) return r;
        HIPC(hipMemcpy(out, dout, ny * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    if (int r = upload(m, dY, ny * 4, (void**)&ddy)) return r;
    float *dgw = nullptr, *dgb = nullptr, *ws = nullptr;
    HIPC(m.out(&dout, nf * 4, "dfeat")); HIPC(m.out(&dgw, nw * 4, "gW")); HIPC(m.out(&dgb, (size_t)O * 4, "gb"));
    HIPC(m.out(&ws, (size_t)512 * (nw + O) * 4, "the slab workspace"));
    HIPC(hipStreamSynchronize(c->stream));          // (the fills run on the context's stream, the copies on the null stream)
    HIPC(hipMemcpy(dgw, gW, nw * 4, hipMemcpyHostToDevice)); HIPC(hipMemcpy(dgb, gb, (size_t)O * 4, hipMemcpyHostToDevice));
    launch_heads_bwd(ddy, dfe, dw, relu_mask != 0, dout, dgw, dgb, ws, n, H, O, c->stream);
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(out, dout, nf * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(gW, dgw, nw * 4, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(gb, dgb, (size_t)O * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The rollout's three sampling kernels (heads.hip) on caller data, any context: (a) launch_heads_sample on feat [n][H], Wh [A + 1][H], bh
// with hout requested and no staging / flag / ticket pointers, (b) launch_sample and (c) launch_logp_all on the hout that (a) wrote.  u [n]
// holds the uniforms, or is NULL and the kernels draw Philox(seed, counter + row).
// Out: act2 [2][n] and logp2 [2][n] of (a), (b); value3 [3][n] of (a), (b), (c); pack [n][3] and hout [n][A + 1] of (a); table [n][A] of (c).
int mi_op_sample(mi_ctx* c, int32_t n, int32_t H, int32_t A, const float* feat, const float* Wh, const float* bh, const float* u, uint64_t seed,
                 uint64_t counter, int32_t value_from_logits, int32_t* act2, float* logp2, float* value3, float* pack, float* hout, float* table) {
    ARG(c && feat && Wh && bh && act2 && logp2 && value3 && pack && hout && table, "null"); JOIN(c);
    ARG(n >= 1 && n <= 65536, "n must be in [1, 65536]"); ARG(A >= 1 && A <= 16, "A must be in [1, 16]"); ARG(H >= 1 && H <= 4096, "H must be in [1, 4096]");
    ARG(value_from_logits == 0 || value_from_logits == 1, "value_from_logits");
    OpMem m("mi_op_sample", c->stream);
    const size_t nh = (size_t)n * (A + 1), N = (size_t)n;
    float *dfe = nullptr, *dw = nullptr, *db = nullptr, *du = nullptr;
    if (int r = upload(m, feat, N * H * 4, (void**)&dfe)) return r;
    if (int r = upload(m, Wh, (size_t)(A + 1) * H * 4, (void**)&dw)) return r;
    if (int r = upload(m, bh, (size_t)(A + 1) * 4, (void**)&db)) return r;
    if (u) { if (int r = upload(m, u, N * 4, (void**)&du)) return r; }
    int32_t* dact[2] = {}; float *dlp[2] = {}, *dval[3] = {}, *dpack = nullptr, *dh = nullptr, *dtab = nullptr;
    static const char* who[3] = {"heads_sample", "sample", "logp_all"};
    for (int k = 0; k < 3; ++k) {
        if (k < 2) { HIPC(m.out(&dact[k], N * 4, (std::string(who[k]) + "'s act").c_str())); HIPC(m.out(&dlp[k], N * 4, (std::string(who[k]) + "'s logp").c_str())); }
        HIPC(m.out(&dval[k], N * 4, (std::string(who[k]) + "'s value").c_str()));
    }
    HIPC(m.out(&dpack, N * 3 * 4, "pack")); HIPC(m.out(&dh, nh * 4, "hout")); HIPC(m.out(&dtab, N * A * 4, "the log-probability table"));
    launch_heads_sample(dfe, dw, db, n, H, A, du, seed, counter, dact[0], dlp[0], dval[0], dpack, dh, nullptr, nullptr, nullptr, c->stream,
                        nullptr, nullptr, 0, value_from_logits);
    launch_sample(dh, n, A, du, seed, counter, dact[1], dlp[1], dval[1], c->stream, value_from_logits);
    launch_logp_all(dh, n, A, dtab, dval[2], c->stream, value_from_logits);
    if (int r = op_finish(c, m)) return r;
    for (int k = 0; k < 3; ++k) {
        if (k < 2) { HIPC(hipMemcpy(act2 + k * N, dact[k], N * 4, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(logp2 + k * N, dlp[k], N * 4, hipMemcpyDeviceToHost)); }
        HIPC(hipMemcpy(value3 + k * N, dval[k], N * 4, hipMemcpyDeviceToHost));
    }
    HIPC(hipMemcpy(pack, dpack, N * 3 * 4, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(hout, dh, nh * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(table, dtab, N * A * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The PPO loss kernels alone (loss.hip) on caller arrays, any context: hout [n][A + 1]; idx [n] into the per-sample arrays act, old_logp,
// old_value, ret, adv [n_rows]; means and gradients scale with 1 / n_global.  fs_coef must be 0 (the feature-sparsity kernels are not run).
//   mode 0: the two-phase path of multi-rank mode 1 on one rank -- launch_loss_fwd, launch_loss_finalize (phase 3), launch_loss_bwd -- the
//           only order in which x_entropy_coef != 0 is legal.  One segment: seg_n / n_seg are not read.
//   mode 1: the one-pass path of mi_minibatch / mi_minibatch_multi -- launch_loss_fwd_seg(with_bwd) + launch_loss_finalize_seg (phase 3, no
//           feature-sparsity parts) over n_seg <= 16 segments of seg_n[k] >= 0 consecutive samples (sum = n); refuses x_entropy_coef != 0.
// Out: dY [n][A + 1]; partial [blocks][8 + A] (columns 0..2 and 8..8+A are written); stats [segments][32] (0..6 and 8..8+A); log [segments][8].
int mi_op_ppo_loss(mi_ctx* c, int32_t mode, int32_t n, int32_t A, const float* hout, const int32_t* idx, int32_t n_rows, const int32_t* act,
                   const float* old_logp, const float* old_value, const float* ret, const float* adv, const mi_hparams* hp,
                   int32_t value_from_logits, int32_t n_global, const int32_t* seg_n, int32_t n_seg, float* dY_out, float* partial_out,
                   float* stats_out, float* log_out) {
    ARG(c && hout && idx && act && old_logp && old_value && ret && adv && hp && dY_out && partial_out && stats_out && log_out, "null"); JOIN(c);
    ARG(mode == 0 || mode == 1, "mode");
    ARG(n >= 1 && n <= 65536 && n_rows >= 1 && n_rows <= (1 << 24), "n must be in [1, 65536], n_rows in [1, 2^24]");
    ARG(A >= 1 && A <= 16, "A must be in [1, 16]"); ARG(n_global >= 1, "n_global");
    ARG(value_from_logits == 0 || value_from_logits == 1, "value_from_logits");
    ARG(hp->fs_coef == 0.f, "fs_coef must be 0: the feature-sparsity kernels are not part of this hook");
    ARG(mode == 0 || hp->x_entropy_coef == 0.f, "mode 1 (the one-pass path) needs x_entropy_coef == 0");
    for (int k = 0; k < n; ++k) ARG(idx[k] >= 0 && idx[k] < n_rows, "index out of range");
    for (int k = 0; k < n_rows; ++k) ARG(act[k] >= 0 && act[k] < A, "action out of range");
    SegTab st{};
    st.n_seg = 1; st.start[1] = n;
    if (mode == 1) {
        ARG(seg_n && n_seg >= 1 && n_seg <= MI_MAX_SEG, "mode 1: 1 .. 16 segments");
        long long tot = 0;
        for (int k = 0; k < n_seg; ++k) { ARG(seg_n[k] >= 0, "negative segment"); tot += seg_n[k]; }
        ARG(tot == n, "segments do not add up to n");
        st.n_seg = n_seg;
        for (int k = 0; k < n_seg; ++k) st.start[k + 1] = st.start[k] + seg_n[k];
    }
    const std::string hook = "mi_op_ppo_loss mode " + std::to_string(mode);
    OpMem m(hook.c_str(), c->stream);
    const size_t nh = (size_t)n * (A + 1);
    const int nblk = mode == 0 ? loss_blocks(n) : loss_blocks_seg(st);
    float *dh = nullptr, *dlp = nullptr, *dov = nullptr, *dret = nullptr, *dadv = nullptr; int32_t *didx = nullptr, *dact = nullptr;
    if (int r = upload(m, hout, nh * 4, (void**)&dh)) return r;
    if (int r = upload(m, idx, (size_t)n * 4, (void**)&didx)) return r;
    if (int r = upload(m, act, (size_t)n_rows * 4, (void**)&dact)) return r;
    if (int r = upload(m, old_logp, (size_t)n_rows * 4, (void**)&dlp)) return r;
    if (int r = upload(m, old_value, (size_t)n_rows * 4, (void**)&dov)) return r;
    if (int r = upload(m, ret, (size_t)n_rows * 4, (void**)&dret)) return r;
    if (int r = upload(m, adv, (size_t)n_rows * 4, (void**)&dadv)) return r;
    LossArgs a{};
    float *stats = nullptr, *log = nullptr;
    HIPC(m.out(&a.dY, nh * 4, "dY")); HIPC(m.out(&a.partial, (size_t)nblk * (8 + A) * 4, "the block partials"));
    HIPC(m.out(&stats, (size_t)st.n_seg * 32 * 4, "the statistics")); HIPC(m.out(&log, (size_t)st.n_seg * 8 * 4, "the log records"));
    a.hout = dh; a.idx = didx; a.act = dact; a.old_logp = dlp; a.old_value = dov; a.ret = dret; a.adv = dadv; a.stats = stats; a.n = n; a.A = A;
    a.inv_n_global = 1.0f / (float)n_global;
    a.value_from_logits = value_from_logits;
    a.hp = LossHP{hp->eps_clip, hp->value_coef, hp->entropy_coef, hp->x_entropy_coef, hp->entropy_multiplier, hp->fs_coef};
    if (mode == 0) {
        launch_loss_fwd(a, c->stream);
        launch_loss_finalize(a, nblk, 3, nullptr, log, c->stream);
        launch_loss_bwd(a, c->stream);
    } else {
        launch_loss_fwd_seg(a, st, true, c->stream);
        launch_loss_finalize_seg(a, st, 3, stats, nullptr, 2048, nullptr, log, c->stream);
    }
    if (int r = op_finish(c, m)) return r;
    HIPC(hipMemcpy(dY_out, a.dY, nh * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(partial_out, a.partial, (size_t)nblk * (8 + A) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(stats_out, stats, (size_t)st.n_seg * 32 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(log_out, log, (size_t)st.n_seg * 8 * 4, hipMemcpyDeviceToHost));
    return 0;
}

// D = A(16x4) * B(4x16) with asymmetric integer data through the operand maps the kernels assume:
// A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15], D[row = (lane>>4)*4 + r][col = lane&15]
__global__ void mfma_selftest_kernel(float* d) {
    const int lane = threadIdx.x, i = lane & 15, q = lane >> 4;
    const float a = (float)(i * 7 + q * 3 + 1), b = (float)(q * 5 - i * 2 + 11);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) d[(q * 4 + r) * 16 + i] = acc[r];
}
int mi_selftest_mfma(mi_ctx* c, float* max_err) {
    ARG(c && max_err, "null"); JOIN(c);
    float* d = nullptr;
    DevPool m(hip_pool());
    HIPC(m.dev(&d, 256));
    hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, c->stream, d);
    HIPC(hipStreamSynchronize(c->stream));
    float h[256];
    HIPC(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    float worst = 0.f;
    for (int m = 0; m < 16; ++m)
        for (int n = 0; n < 16; ++n) {
            float ref = 0.f;
            for (int k = 0; k < 4; ++k) ref += (float)(m * 7 + k * 3 + 1) * (float)(k * 5 - n * 2 + 11);
            worst = fmaxf(worst, fabsf(ref - h[m * 16 + n]));
        }
    *max_err = worst;
    return 0;
}
