// bf16 MFMA GEMM with fused epilogue for gfx950 (CDNA4).
//
//   C[M,N] = epilogue( alpha * sum_k opA[m,k] * opB[n,k] )
//
// Replaces every nn.Linear / conv-as-GEMM contraction on the Prismer hot path:
//   forward   x[M,K] . W[N,K]^T            (both K-contiguous)               -> trans_a=0, trans_b=0
//   dgrad     dY[M,N'] . W[N',K']          (W stored [red][out])             -> trans_a=0, trans_b=1
//   wgrad     dY[M',N]^T . X[M',K]         (both stored [red][out])          -> trans_a=1, trans_b=1
// reference call sites: vit.py:41-47,53 (ViT), resampler.py:18-24, utils.py:50-56 (Adaptor),
// roberta.py:86-92,134,163,177,415-421 (decoder), vit.py:86-120 (convs lowered to im2col GEMMs).
//
// Design (wave64, MFMA 32x32x16 bf16, fp32 accumulate) -- details and measurements in DESIGN.md section 3:
//   * block = 256 threads = 4 waves in a 2x2 grid; block tile 128x128 or 64x64 (cost model on the host), BK = 64.
//   * operands staged global -> VGPR -> LDS (double buffer, one barrier per k-tile); the registers of tile t+1 are
//     written to LDS right after the barrier and immediately re-issued for tile t+2 (two tiles of look-ahead).
//   * K-contiguous operand: LDS image [rows][64] bf16 (128-B rows), 16-B chunk index XOR-swizzled with (row>>1)&7 so
//     the ds_read_b128 fragment reads of a 16-lane group hit 16 distinct 16-B slots.
//   * K-strided operand (stored [K][rows]): LDS image [64][rows] with a 64-B row pad, fragments fetched with the gfx950
//     transposing LDS read ds_read_b64_tr_b16 (two per 8-element fragment) -- no transposed copies anywhere.
//   * epilogue through LDS (row-contiguous 16-B vectors), fused bias / activation / act' / dropout / residual / accumulate.
//   * split-K (grid.z): partial tiles to an fp32 workspace + splitk_reduce_kernel (which runs the same epilogue).
//   * XCD-aware, grouped tile rasterisation (each XCD walks 8-row-panel groups, rows fastest).
#include "gemm_common.h"
#include <algorithm>
#include <vector>

using namespace phg;

namespace {

// folds the split-K partials and applies the fused epilogue (bias / activation / dropout / residual / accumulate / dtype).
// LANES threads share one output vector: lane l sums the splits l, l + LANES, ... and the group is folded with shuffles -- with up to
// 256 splits of a tiny output (the stems' first-layer weight gradients: 768 output vectors) one thread per vector walked 256
// dependent loads (62 us for 3 blocks); 16 lanes per vector make it 16 loads and 48 blocks.
template <int LANES>
__device__ __forceinline__ void splitk_reduce_body(const GemmParams& p, const int splits, const int block, const int nblocks) {
  const int n4 = (p.N + 3) / 4;
  int64_t total = (int64_t)p.M * n4;
  DropCtx dc;
  const bool drop = p.drop_p > 0.0f;
  if (drop) dc = make_drop(p.drop_seed, p.drop_stream, p.drop_p);
  const int sub = threadIdx.x % LANES;
  // (the LANES lanes of a group share `id`, hence their control flow: the shuffles below always see the whole group)
  for (int64_t id = ((int64_t)block * 256 + threadIdx.x) / LANES; id < total; id += (int64_t)nblocks * (256 / LANES)) {
    int m = (int)(id / n4), n = (int)(id % n4) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = sub; s < splits; s += LANES) acc += *reinterpret_cast<const f32x4*>(p.ws + ((size_t)s * p.M + m) * p.ldws + n);
    if constexpr (LANES > 1) {
#pragma unroll
      for (int o = LANES / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
      }
    }
    if (sub == 0) {
      float v[4] = {acc[0], acc[1], acc[2], acc[3]};
      epilogue_store(p, m, n, v, false, drop, dc);
    }
  }
}
template <int LANES>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmParams p, int splits) {
  splitk_reduce_body<LANES>(p, splits, blockIdx.x, gridDim.x);
}
// the fold passes of several deferred split-K GEMMs in one grid (ph_gemm_args.defer_reduce / ph_gemm_flush_deferred)
struct ReduceGroup {
  int n;
  int blk_start[PH_GEMM_GROUP_MAX + 1];
  int splits[PH_GEMM_GROUP_MAX];
  GemmParams p[PH_GEMM_GROUP_MAX];
};
template <int LANES>
__global__ __launch_bounds__(256) void splitk_reduce_grouped_kernel(ReduceGroup g) {
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.blk_start[i + 1]) ++i;
  splitk_reduce_body<LANES>(g.p[i], g.splits[i], (int)blockIdx.x - g.blk_start[i], g.blk_start[i + 1] - g.blk_start[i]);
}

}  // namespace


namespace phg { std::atomic<long long> g_gemm_counts[PH_GEMM_CLS_COUNT]; }
// run-time tuning (ph_gemm_tuning); -1 = not set yet: the first reader takes the environment default
static std::atomic<int> g_big_mode{-1}, g_big_min_tiles{-1};      // (read by tuning_now below)

// ---- deferred fold passes (ph_gemm_args.defer_reduce): one queue per process, see the header for the calling contract
namespace {
struct DeferredReduce { GemmParams p; int splits; bool wide; };    // wide: the 16-lanes-per-vector form
std::mutex g_defer_mu;
std::vector<DeferredReduce> g_defer;
size_t g_defer_cursor = 0;              // bytes of the caller's workspace taken by the queued partial sums
const void* g_defer_ws = nullptr;

int reduce_blocks(const GemmParams& p, bool wide) {
  const int64_t vecs = (int64_t)p.M * ((p.N + 3) / 4);
  return (int)std::min<int64_t>(2048, ceil_div64(wide ? vecs * 16 : vecs, 256));
}
int flush_deferred_locked(hipStream_t stream) {
  for (int wide = 0; wide < 2; ++wide) {
    size_t i = 0;
    while (true) {
      ReduceGroup g;
      g.n = 0; g.blk_start[0] = 0;
      for (; i < g_defer.size() && g.n < PH_GEMM_GROUP_MAX; ++i) {
        if ((int)g_defer[i].wide != wide) continue;
        g.p[g.n] = g_defer[i].p; g.splits[g.n] = g_defer[i].splits;
        g.blk_start[g.n + 1] = g.blk_start[g.n] + reduce_blocks(g_defer[i].p, wide != 0);
        ++g.n;
      }
      if (g.n == 0) break;
      count_launch(PH_GEMM_CLS_SPLITK_REDUCE);
      if (wide) hipLaunchKernelGGL(splitk_reduce_grouped_kernel<16>, dim3(g.blk_start[g.n]), dim3(256), 0, stream, g);
      else hipLaunchKernelGGL(splitk_reduce_grouped_kernel<1>, dim3(g.blk_start[g.n]), dim3(256), 0, stream, g);
      PH_LAUNCH_CHECK("splitk_reduce_grouped_kernel");
    }
  }
  g_defer.clear();
  g_defer_cursor = 0;
  g_defer_ws = nullptr;
  return PH_OK;
}
}  // namespace


extern "C" int ph_gemm_flush_deferred(hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_defer_mu);
  if (g_defer.empty()) return PH_OK;
  return flush_deferred_locked(stream);
}

extern "C" int ph_gemm_tuning(int big_mode, int big_min_tiles) {
  if (big_mode >= 0) g_big_mode.store(big_mode, std::memory_order_relaxed);
  if (big_min_tiles >= 0) g_big_min_tiles.store(big_min_tiles, std::memory_order_relaxed);
  return PH_OK;
}

extern "C" int ph_gemm_dispatch_counts(int64_t* out, int n, int reset) {
  PH_CHECK_ARG(n >= 0 && (out || n == 0), "ph_gemm_dispatch_counts: null output");
  for (int i = 0; i < PH_GEMM_CLS_COUNT; ++i) {
    const long long v = reset ? g_gemm_counts[i].exchange(0, std::memory_order_relaxed) : g_gemm_counts[i].load(std::memory_order_relaxed);
    if (i < n) out[i] = (int64_t)v;
  }
  return PH_GEMM_CLS_COUNT;
}

// device-resident zero vector standing in for a null bias (epilogue classes, gemm_common.h): part of the code object, no allocation
static __device__ float g_zero_bias[PH_ZERO_BIAS_FLOATS];
// (the address of a __device__ array is PER DEVICE: cached per device id -- a process that launches on a second GPU must not hand it the first
// GPU's address; round-4 advisor finding)
static const float* zero_bias_ptr() {
  constexpr int MAX_DEV = 64;
  static std::atomic<const float*> cache[MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  const float* ptr = cache[dev].load(std::memory_order_acquire);
  if (!ptr) {
    void* d = nullptr;
    if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_zero_bias)) != hipSuccess) return nullptr;
    ptr = static_cast<const float*>(d);
    cache[dev].store(ptr, std::memory_order_release);
  }
  return ptr;
}

// argument validation + kernel parameter block shared by the single and the grouped entry point
static int fill_params(const ph_gemm_args* a, GemmParams& p) {
  PH_CHECK_ARG(a && a->A && a->B && a->C, "ph_gemm_bf16: null pointer");
  PH_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "ph_gemm_bf16: bad dims M=%d N=%d K=%d", a->M, a->N, a->K);
  PH_CHECK_ARG(((a->lda % 8) == 0 || (a->conv && !a->trans_a)) && ((a->ldb % 8) == 0 || (a->conv && a->trans_b)),
               "ph_gemm_bf16: lda/ldb must be multiples of 8 (16-B rows)");
  PH_CHECK_ARG((((uintptr_t)a->A | (uintptr_t)a->B) & 15) == 0, "ph_gemm_bf16: A/B must be 16-B aligned");
  PH_CHECK_ARG(a->trans_a || a->trans_b || (a->K % 8) == 0, "ph_gemm_bf16: K %% 8 != 0 needs a K-strided operand");
  PH_CHECK_ARG((a->lda >= (a->trans_a ? a->M : a->K) || (a->conv && !a->trans_a)) && (a->ldb >= (a->trans_b ? a->N : a->K) || (a->conv && a->trans_b)) &&
               a->ldc >= a->N, "ph_gemm_bf16: leading dimension too small");
  PH_CHECK_ARG(!(a->drop_p > 0.0f) || ((a->N % 4) == 0 && a->drop_seed), "ph_gemm_bf16: dropout needs N %% 4 == 0 and a seed");
  PH_CHECK_ARG(a->drop_p >= 0.0f && a->drop_p < 1.0f, "ph_gemm_bf16: bad dropout p");
  p.A = (const bf16*)a->A; p.B = (const bf16*)a->B; p.C = a->C;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
  p.bias = a->bias; p.bias_or_zero = a->bias ? a->bias : (a->N <= PH_ZERO_BIAS_FLOATS ? zero_bias_ptr() : nullptr);
  p.zero16 = reinterpret_cast<const bf16*>(zero_bias_ptr());
  p.pre_out = (bf16*)a->pre_out; p.act_in = (const bf16*)a->act_in; p.ld_act = a->ld_act;
  p.residual = (const bf16*)a->residual; p.ldr = a->ldr; p.res_f32 = a->residual_f32;
  p.drop_p = a->drop_p; p.drop_seed = a->drop_seed; p.drop_stream = a->drop_stream;
  p.act = a->act; p.out_f32 = a->out_f32; p.accumulate = a->accumulate; p.alpha = a->alpha; p.pre_grad = a->pre_grad;
  p.ws = nullptr; p.ldws = (a->N + 3) / 4 * 4;
  p.col_stats = a->col_stats;
  PH_CHECK_ARG(!a->a_colsum || (a->trans_a && a->trans_b && !a->conv), "ph_gemm_bf16: a_colsum needs the [K][M] x [K][N] layout without a conv gather");
  p.a_colsum = a->a_colsum; p.tile_cnt = nullptr;
  p.cv = ConvGather{};
  p.rm_wo = a->rowmap_wo; p.rm_mul = a->rowmap_mul; p.rm_sub = a->rowmap_sub; p.rm_add = a->rowmap_add;
  p.rm_inv_wo = a->rowmap_wo > 0 ? 1.0f / (float)a->rowmap_wo : 0.f;
  PH_CHECK_ARG(a->rowmap_wo >= 0 && (a->rowmap_wo == 0 || (!a->pre_out && !a->accumulate && a->split_k <= 1 && a->M < (1 << 24) && a->rowmap_mul >= 1 && a->rowmap_sub >= 0)),
               "ph_gemm_bf16: output row map needs a plain store epilogue (no pre_out / accumulate / split-K) and M < 2^24");
  if (a->conv) {
    const ph_conv_gather& c = *a->conv;
    const bool general = c.kh > 0;
    PH_CHECK_ARG(c.B > 0 && c.H > 0 && c.W > 0 && c.C > 0 && (c.C % 8) == 0 && (general || c.ks == 1 || c.ks == 3) && c.stride >= 1,
                 "ph_gemm_bf16: bad conv gather (C %% 8 == 0, ks 1 or 3)");
    PH_CHECK_ARG(!general || (c.kh >= 1 && c.kh <= 3 && c.kw >= 1 && c.kw <= 3 && c.Ho > 0 && c.Wo > 0 && !a->trans_a && !a->trans_b),
                 "ph_gemm_bf16: generalised conv window: 1..3 x 1..3 taps, forward-shaped gather only");
    const int pad = c.ks / 2;
    const int Ho = general ? c.Ho : (c.H + 2 * pad - c.ks) / c.stride + 1, Wo = general ? c.Wo : (c.W + 2 * pad - c.ks) / c.stride + 1;
    const int64_t rows = (int64_t)c.B * Ho * Wo;
    PH_CHECK_ARG(rows < (1 << 24) && (int64_t)c.B * c.H * c.W < (1ll << 31) / 1, "ph_gemm_bf16: conv gather index space too large");
    const int Kreal = general ? c.kh * c.kw * c.C : c.ks * c.ks * c.C;
    if (!a->trans_a && !a->trans_b) PH_CHECK_ARG(a->M == rows && a->K >= Kreal && (a->K % 8) == 0, "ph_gemm_bf16: conv A: M must be B*Ho*Wo (%lld), K >= ks*ks*C", (long long)rows);
    else if (a->trans_a && a->trans_b) PH_CHECK_ARG(a->K == rows && a->N >= Kreal, "ph_gemm_bf16: conv B: K must be B*Ho*Wo (%lld), N >= ks*ks*C", (long long)rows);
    else return ph_fail(PH_ERR_UNSUPPORTED, "ph_gemm_bf16: conv gather is defined for the NN (forward) and TT (weight gradient) layouts");
    p.cv.H = c.H; p.cv.W = c.W; p.cv.C = c.C; p.cv.ks = c.ks; p.cv.stride = c.stride; p.cv.Ho = Ho; p.cv.Wo = Wo; p.cv.Kreal = Kreal;
    p.cv.inv_howo = 1.0f / (float)(Ho * Wo); p.cv.inv_wo = 1.0f / (float)Wo; p.cv.inv_c = 1.0f / (float)c.C;
    p.cv.kh = general ? c.kh : c.ks; p.cv.kw = general ? c.kw : c.ks; p.cv.offy = general ? c.off_y : -pad; p.cv.offx = general ? c.off_x : -pad;
  }
  PH_CHECK_ARG(!a->col_stats || (!a->bias && a->act == PH_ACT_NONE && !a->act_in && !a->residual && !(a->drop_p > 0.f) && !a->accumulate),
               "ph_gemm_bf16: col_stats needs a plain epilogue");
  return PH_OK;
}

// ================================================================================================================================
// Dispatch: decide the route first, launch second.  route_single / route_grouped turn (arguments, tuning) into a Route -- kernel class, tile,
// variant, per-problem k split, grid, fold pass, workspace layout -- with no HIP call, lock, counter or profiler (they run on a machine without
// a device; ph_gemm_route hands the same value to the host); ph_gemm_bf16 / run_grouped execute a Route.  The rules in order: DESIGN.md section 3.

// ---- fitted constants of the cost models (us; time of a launch = rounds x (fixed + k-tiles x per-k-tile)) -- every one named once.
// The fixed parts of the single and of the grouped models DIFFER for what looks like the same quantity (12.0 / 14.0 for a 256x128 block, 12.0 /
// 10.0 for a 128x128 round): each was fitted with its own dispatch rule and nobody has re-measured which is right, so both stay, under two names.
namespace fit {
// per-shape fit of DESIGN.md section 3 ("What the per-shape fit says about ALL these GEMMs"; profiles/r2_gemm_by_grid.txt)
constexpr double BIG_KTILE = 0.67;            // a 256x128 LDS-DMA block alone on its CU
// the same block with B gathered from an activation (CONV = 2).  Measured side by side on one uncut group (tools/stem_wgrad_probe.py,
// profiles/stem_wgrad_ktile.txt): 0.881 us per k-tile gathered against 0.792 us plain, i.e. the gather costs the loop 11 %.  That probe's plain
// figure is not the 0.67 of the per-shape fit every other constant here was fitted beside, so the SURCHARGE is what is used: 0.67 x 0.881 / 0.792
constexpr double BIG_KTILE_GATHER = 0.745;
constexpr double PAIR128_KTILE = 0.84;        // a pair of co-resident 128x128 blocks
constexpr double LONE128_KTILE = 0.5;         // a lone 128x128 block (the last, half-empty round)
constexpr double BIG_FIXED_SINGLE = 12.0, R128_FIXED_SINGLE = 12.0;          // ph_gemm_bf16: 256x128 against 128x128
constexpr double NN_TIE = 1.02;               // ties go to the 256x128 kernel for [N,K] B (stem 25088x384x1728), against it for [K,N] B (LARGE dgrads)
// the persistent weight-gradient plan (k-balanced plan): prologue + parking + write-out of a unit, slab write + read-back
constexpr double BIG_FIXED_GROUPED = 14.0, BIG_SLAB = 6.0, R128_FIXED_GROUPED = 10.0;
// register-staged tile / split-K model: slope probe 8320x768 NT, K 768 -> 3072 (profiles/r1_*): one wave of co-resident 128x128 blocks (2 per CU),
// of 64x64 blocks (4 per CU), fixed part of a block wave; fold launch measured with rocprof + partial traffic in bytes per us
constexpr double REG128_KTILE = 1.07, REG64_KTILE = 0.83, REG_WAVE_FIXED = 4.0, FOLD_LAUNCH = 8.0, FOLD_BYTES_PER_US = 3.0e6;
}  // namespace fit
// Floor of the persistent plan: a unit shorter than BIG_FIXED_GROUPED / BIG_KTILE = 21 k-tiles spends more time in the fixed part than in its k
// loop, and every further cut ADDS more fixed time to the chip than it removes loop time from the longest block -- no k-range is shorter.
constexpr int BIG_KT_FLOOR = 21, BIG_MAX_SPLIT = 32, BIG_MAX_UNITS = 8192;
static_assert(BIG_KT_FLOOR * fit::BIG_KTILE >= fit::BIG_FIXED_GROUPED && (BIG_KT_FLOOR - 1) * fit::BIG_KTILE < fit::BIG_FIXED_GROUPED, "floor = fixed part / k-tile time");
constexpr int SLOTS128 = 512, SLOTS64 = 1024;      // co-resident blocks of the chip: 2 x 128x128 or 4 x 64x64 per CU

struct Tuning { int big_mode, big_min_tiles; bool zero_page; };      // zero_page: zero_bias_ptr() is there (the LDS-DMA conv gather reads it)
static Tuning tuning_now(bool device) {
  int m = g_big_mode.load(std::memory_order_relaxed), t = g_big_min_tiles.load(std::memory_order_relaxed);
  return Tuning{m < 0 ? 7 : m, t < 0 ? 128 : t, !device || zero_bias_ptr() != nullptr};
}

constexpr int GMAX = PH_GEMM_GROUP_MAX;
struct Route {
  int cls = PH_GEMM_CLS_GROUPED, bm = 0, bn = 0;
  BigVariant variant = BigVariant::off;            // 256x128 kernels only
  int ta = 0, tb = 0, pf = 0, conv = 0;            // as the register-staged grouped launchers take them (pf: prefetch ring; conv: 1 gathered A, 2 gathered B)
  int n = 1, max_blocks = 0;
  int tiles_m[GMAX], tiles_n[GMAX], nsplit[GMAX], kt_per_split[GMAX];
  int start[GMAX + 1];                                // first block (persistent kernel: unit) of problem i; start[n] = blocks / units of the launch
  int max_split = 1;
  int fold = PH_GEMM_FOLD_NONE, fold_lanes = 0;
  size_t ws_bytes = 0, cnt_bytes = 0;              // workspace: arrival counters of all cut problems first (cnt_bytes), partial sums / slabs behind
  size_t cnt_off[GMAX], ws_off[GMAX];
  int tail_m = 0;                                  // ph_gemm_bf16: > 0 = the call is two calls, rows [0, tail_m) and [tail_m, M); nothing else is set
  bool as_group = false;                           // ph_gemm_bf16: served as a group of one (conv NN, a_colsum)
};

static bool plain_f32(const ph_gemm_args& a) {     // the write-out a k split can fold: alpha x acc (+ C) in fp32
  return a.out_f32 && !a.bias && a.act == PH_ACT_NONE && !a.pre_out && !a.act_in && !a.residual && !(a.drop_p > 0.f);
}
static int tiles_of(const ph_gemm_args& a, int bm, int bn) { return ceil_div(a.M, bm) * ceil_div(a.N, bn); }

// ---- plan of a weight-gradient group on the persistent 256x128 kernel ---------------------------------------------------------
// The kernel's 256 blocks walk the units of the group in order, block b takes units b, b + 256, ...; a unit is (problem, tile, k-range).
// Cost of a unit: BIG_KTILE per k-tile + BIG_FIXED_GROUPED; a unit of a tile that is cut over K also writes its fp32 tile as a slab and one
// unit per tile reads them all back: + BIG_SLAB.  The makespan is the longest block.  Unsplit, a group of T tiles costs ceil(T / 256) rounds
// whatever T % 256 is; cutting every tile of problem i into ns_i k-ranges lets the units of the whole group fill the rounds evenly.
struct BigPlan { int ns[GMAX]; int units, max_split; double cost; size_t ws_bytes; };

static double big_makespan(const ph_gemm_args* args, int n, const int* ns, double ktile, int* units_out) {
  double load[256];
  for (int b = 0; b < 256; ++b) load[b] = 0.0;
  int u = 0;
  for (int i = 0; i < n; ++i) {
    const int tiles = tiles_of(args[i], big::BM, big::BN), kt = args[i].K / BK;
    for (int sp = 0; sp < ns[i]; ++sp) {
      const int len = kt / ns[i] + (sp < kt % ns[i] ? 1 : 0);
      const double c = len * ktile + fit::BIG_FIXED_GROUPED + (ns[i] > 1 ? fit::BIG_SLAB : 0.0);
      for (int t = 0; t < tiles; ++t, ++u) load[u & 255] += c;
    }
  }
  double worst = 0.0;
  for (int b = 0; b < 256; ++b) worst = load[b] > worst ? load[b] : worst;
  *units_out = u;
  return worst;
}
// bytes of workspace per cut problem: one int counter per tile (256-B aligned block) + tiles x ns slabs of 256 x 128 fp32
static size_t big_cnt_bytes(int tiles) { return ((size_t)tiles * 4 + 255) / 256 * 256; }
static size_t big_slab_bytes(int tiles, int ns) { return (size_t)tiles * ns * (size_t)(big::BM * big::BN * 4); }
static BigPlan plan_big_wgrad(const ph_gemm_args* args, int n, bool may_split, double ktile) {
  BigPlan best;
  int tiles_all = 0, kt_max = 0;
  for (int i = 0; i < n; ++i) {
    best.ns[i] = 1;
    tiles_all += tiles_of(args[i], big::BM, big::BN);
    kt_max = std::max(kt_max, args[i].K / BK);
  }
  best.max_split = 1; best.ws_bytes = 0;
  best.cost = big_makespan(args, n, best.ns, ktile, &best.units);
  // groups that fill whole rounds stay as they are
  if (!may_split || tiles_all % 256 == 0) return best;
  // candidate c: k-ranges of about kt_max / c k-tiles for every problem of the group
  for (int c = 2; c <= BIG_MAX_SPLIT && kt_max / c >= BIG_KT_FLOOR; ++c) {
    BigPlan pl;
    const double L = (double)kt_max / c;
    pl.max_split = 1; pl.ws_bytes = 0;
    for (int i = 0; i < n; ++i) {
      const int kt = args[i].K / BK;
      pl.ns[i] = std::max(1, std::min({(int)lround(kt / L), kt / BIG_KT_FLOOR, BIG_MAX_SPLIT}));
      pl.max_split = std::max(pl.max_split, pl.ns[i]);
      const int tiles = tiles_of(args[i], big::BM, big::BN);
      if (pl.ns[i] > 1) pl.ws_bytes += big_cnt_bytes(tiles) + big_slab_bytes(tiles, pl.ns[i]);
    }
    if (pl.ws_bytes > (size_t)args[0].workspace_bytes) continue;
    pl.cost = big_makespan(args, n, pl.ns, ktile, &pl.units);
    if (pl.units <= BIG_MAX_UNITS && pl.cost < best.cost) best = pl;
  }
  return best;
}

// whole problems on bm x bn tiles, one block per tile: what every grouped route starts from
static void whole_tiles(Route& r, const ph_gemm_args* args, int bm, int bn) {
  r.bm = bm; r.bn = bn; r.max_split = 1;
  int tot = 0;
  for (int i = 0; i < r.n; ++i) {
    r.tiles_m[i] = ceil_div(args[i].M, bm); r.tiles_n[i] = ceil_div(args[i].N, bn);
    r.nsplit[i] = 1; r.kt_per_split[i] = ceil_div(args[i].K, BK);
    r.start[i] = tot;
    tot += r.tiles_m[i] * r.tiles_n[i];
  }
  r.start[r.n] = tot;
}

static Route route_grouped(const ph_gemm_args* args, int n, int max_blocks, const Tuning& t) {
  Route r;
  r.n = n; r.max_blocks = max_blocks; r.ta = args[0].trans_a; r.tb = args[0].trans_b;
  const bool conv = args[0].conv != nullptr, tt = r.ta && r.tb;
  const BigVariant big = big_variant(t.big_mode);
  int kt_max = 0, t128 = 0;
  bool kfull = true, thin = false;
  // one workspace for the whole group and plain fp32 write-outs: what either k split needs
  bool shared_ws = args[0].workspace && args[0].workspace_bytes > 0;
  for (int i = 0; i < n; ++i) {
    const ph_gemm_args& a = args[i];
    kt_max = std::max(kt_max, ceil_div(a.K, BK));
    t128 += tiles_of(a, 128, 128);
    kfull = kfull && (a.K % BK) == 0;
    thin = thin || a.M <= 64 || a.N <= 64;
    shared_ws = shared_ws && a.workspace == args[0].workspace && plain_f32(a) && !a.col_stats && a.rowmap_wo == 0;
  }
  // 128x128 tiles (twice the arithmetic intensity per staged byte) unless the group is so small that they would leave most
  // CUs idle; long reductions always take them (measured: 16 adaptor wgrads 768x384xK=8320 ran 440 us on 64x64 tiles)
  const int bsel = (!thin && (t128 >= 192 || (kt_max >= 32 && t128 >= 64))) ? 128 : 64;
  whole_tiles(r, args, bsel, bsel);
  const int total = r.start[n];

  // ---- weight-gradient groups with long reductions: the 256x128 ping-pong kernel, one persistent block per CU, units = (tile, k-range) ----
  BigPlan plan;
  bool use_big = false, big_first = false;
  {
    // a gathered B (the stems' 3x3 weight gradients: B = im2col view, k-row = output pixel) rides on the same units: the gather is the DMA
    // source address, padding reads the zero page, element offsets are 32-bit
    bool ok = big != BigVariant::off && (!conv || t.zero_page) && max_blocks == 0 && tt;
    bool roomy = true;            // every problem covers at least one whole 256x128 tile
    int kt_min = 1 << 30;
    for (int i = 0; i < n && ok; ++i) {
      const ph_gemm_args& a = args[i];
      ok = (a.K % BK) == 0 && (a.M % 8) == 0 && (a.N % 8) == 0 && a.M >= 8 && a.N >= 8 && !a.col_stats;
      if (ok && conv) {
        const ph_conv_gather& c = *a.conv;
        ok = c.kh == 0 && (c.ks == 1 || c.ks == 3) && c.C > 0 && (c.C % 8) == 0 && !a.a_colsum && !(a.drop_p > 0.f) && c.H < (1 << 20) &&
             (int64_t)c.B * c.H * c.W * c.C < (1ll << 31);
      }
      roomy = roomy && a.M >= big::BM && a.N >= big::BN;
      kt_min = std::min(kt_min, a.K / BK);
    }
    if (ok && kt_min >= 32) {
      // makespan of the persistent kernel under its best plan against rounds x (k loop + fixed part) of the 128x128 grouped kernel
      plan = plan_big_wgrad(args, n, shared_ws, conv ? fit::BIG_KTILE_GATHER : fit::BIG_KTILE);
      const double cost_128 = bsel != 128 ? 1e30 : total <= 256 ? kt_max * fit::LONE128_KTILE + fit::R128_FIXED_GROUPED
                                                                : ceil(total / (double)SLOTS128) * (kt_max * fit::PAIR128_KTILE + fit::R128_FIXED_GROUPED);
      use_big = plan.cost < cost_128;
      // a cut plan over whole tiles goes ahead of the register-staged split below (which is for outputs far smaller than a 256x128 tile:
      // the stems' 96 x 32 weight gradients)
      big_first = use_big && plan.max_split > 1 && roomy;
    }
  }
  auto take_big = [&]() {
    whole_tiles(r, args, big::BM, big::BN);
    r.cls = PH_GEMM_CLS_BIG_GROUPED; r.variant = big == BigVariant::spread ? BigVariant::spread : BigVariant::lean;
    r.max_split = plan.max_split; r.fold = plan.max_split > 1 ? PH_GEMM_FOLD_IN_LAUNCH : PH_GEMM_FOLD_NONE;
    r.conv = conv ? 2 : 0;
    int tot = 0;
    for (int i = 0; i < n; ++i) {
      const int tiles = r.tiles_m[i] * r.tiles_n[i];
      r.nsplit[i] = plan.ns[i]; r.kt_per_split[i] = ceil_div(args[i].K / BK, plan.ns[i]);
      if (plan.ns[i] > 1) { r.cnt_off[i] = r.cnt_bytes; r.cnt_bytes += big_cnt_bytes(tiles); }
      r.start[i] = tot;
      tot += tiles * plan.ns[i];
    }
    r.start[n] = tot;
    r.ws_bytes = r.cnt_bytes;
    for (int i = 0; i < n; ++i) {
      if (plan.ns[i] > 1) { r.ws_off[i] = r.ws_bytes; r.ws_bytes += big_slab_bytes(r.tiles_m[i] * r.tiles_n[i], plan.ns[i]); }
    }
    return r;
  };
  if (big_first) return take_big();
  // ---- grouped AND split over K: weight-gradient groups with few output tiles and very long reductions -- the stems' conv weight
  // gradients, 6 experts x (2..42 tiles over up to 6272 k-tiles).  Every problem is cut into pieces of ~W/slots k-tiles so that the whole
  // group fills the chip once, partial sums go to the caller's workspace and ONE grouped pass folds them (plain fp32 epilogues only).
  const int slots = bsel == 128 ? SLOTS128 : SLOTS64;
  if (max_blocks == 0 && tt && shared_ws && total * 2 <= slots) {
    double W = 0.0;
    for (int i = 0; i < n; ++i) W += (double)r.tiles_m[i] * r.tiles_n[i] * ceil_div(args[i].K, BK);
    const int L = std::max(8, (int)ceil(W / slots));            // k-tiles per block
    int nsp[GMAX], max_split = 1;
    size_t off = 0, offs[GMAX];
    for (int i = 0; i < n; ++i) {
      const int kti = ceil_div(args[i].K, BK);
      const int ns = std::min(ceil_div(kti, L), std::max(1, kti / 4));
      nsp[i] = ceil_div(kti, ceil_div(kti, std::max(1, ns)));
      offs[i] = off;
      if (nsp[i] > 1) off += ((size_t)nsp[i] * args[i].M * ((args[i].N + 3) / 4 * 4) * 4 + 255) / 256 * 256;
      max_split = std::max(max_split, nsp[i]);
    }
    if (max_split > 1 && off <= (size_t)args[0].workspace_bytes) {
      if (conv && use_big) {
        // gathered groups choose between the two k splits by modelled cost, not by rule order (layer 2 of the stems, M = 192, is not "roomy" and
        // still far cheaper on the persistent units): one wave of co-resident register-staged blocks of L k-tiles + the fold pass and its traffic
        double part_bytes = 0.0;
        for (int i = 0; i < n; ++i) part_bytes += nsp[i] > 1 ? (double)nsp[i] * args[i].M * ((args[i].N + 3) / 4 * 4) * 4.0 : 0.0;
        const double cost_split = L * (bsel == 128 ? fit::REG128_KTILE : fit::REG64_KTILE) + fit::REG_WAVE_FIXED + fit::FOLD_LAUNCH + part_bytes / fit::FOLD_BYTES_PER_US;
        if (plan.cost < cost_split) return take_big();
      }
      int tot = 0;
      for (int i = 0; i < n; ++i) {
        r.nsplit[i] = nsp[i]; r.kt_per_split[i] = ceil_div(ceil_div(args[i].K, BK), nsp[i]); r.ws_off[i] = offs[i];
        r.start[i] = tot;
        tot += r.tiles_m[i] * r.tiles_n[i] * nsp[i];
      }
      r.start[n] = tot;
      r.pf = 0; r.conv = conv ? 2 : 0;
      r.max_split = max_split; r.ws_bytes = off; r.fold = PH_GEMM_FOLD_PASS; r.fold_lanes = 1;
      return r;
    }
  }
  if (use_big) return take_big();
  // ---- forward-shaped implicit convolutions with many rows and a long reduction (the stems' layers 2..4 and their data gradients): the
  // 256x128 LDS-DMA kernel with the gather in the DMA source address (the register-staged gather kernel ran them at ~410 TFLOP/s)
  if (conv && !r.ta && !r.tb && t.big_mode > 1 && max_blocks == 0) {
    bool ok = t.zero_page;                                   // the gather's padding lanes read the zero page
    for (int i = 0; i < n && ok; ++i) {
      const ph_gemm_args& a = args[i];
      ok = a.M >= big::BM && a.K >= 2 * BK && (a.N % 8) == 0 && a.N >= 8 && (a.ldb % 8) == 0 && a.split_k <= 1 &&
           (int64_t)a.conv->B * a.conv->H * a.conv->W * a.conv->C < (1ll << 31);          // 32-bit element offsets in the gather
    }
    if (ok) {
      whole_tiles(r, args, big::BM, big::BN);
      r.cls = PH_GEMM_CLS_BIG_GROUPED; r.variant = big == BigVariant::spread ? BigVariant::spread : BigVariant::lean; r.conv = 1;
      int blocks = 0;
      for (int i = 0; i < n; ++i) {
        r.start[i] = blocks;
        blocks += big_xcd_grid(r.tiles_m[i], r.tiles_n[i]);          // (XCD shares, see big_tile: the blocks beyond a share exit)
      }
      r.start[n] = blocks;
      return r;
    }
  }
  // ---- register-staged grouped kernel, whole problems.  Gathered operand: forward (NN, A = im2col view, through the prefetch ring: the gather
  // loads are unconditional, so the ring's straight-line bookkeeping holds for any K) or weight gradient (TT, B = im2col view, no ring); plain
  // problems take the ring whenever every K is a multiple of BK
  if (conv) { r.conv = r.ta ? 2 : 1; r.pf = r.ta ? 0 : 1; r.ta = r.tb = r.ta ? 1 : 0; }
  else r.pf = kfull ? 1 : 0;
  return r;
}

// ---- tail split: a launch whose tile count is a little above a whole number of block rounds pays a full extra round for a handful of tiles
// (c_fc 8320 x 3072: 65 x 24 = 1560 tiles of 128x128 on 512 block slots = 3.05 rounds -> 4 tile times, ~95 us).  The rows that cause the
// overshoot (the last, partial row panels) are cut off and computed by a second, small call: 8192 x 3072 = exactly 3 rounds (+ 128 x 3072 on
// 64x64 tiles, ~10 us beside an otherwise idle chip).  Returns the first row of the second call, 0 = no split.
static int tail_split_row(const ph_gemm_args& a) {
  const int64_t tn128 = ceil_div(a.N, 128), tiles = (int64_t)ceil_div(a.M, 128) * tn128, slots = SLOTS128;
  if (a.trans_a || a.conv || a.col_stats || a.drop_p > 0.0f || a.split_k > 0 || a.rowmap_wo != 0 || tiles <= slots || (a.K % BK) != 0) return 0;
  const int64_t over = tiles % slots;
  const int64_t m_main = (tiles / slots) * slots / tn128 * 128, m_rem = a.M - m_main;      // the row panels that fit the whole rounds
  // worth it when the overshoot is small (<= 12 % of a round) and the cut-off part is itself a small problem
  return (over > 0 && over * 100 <= slots * 12 && m_rem > 0 && m_rem <= 512 && (m_main % 256) == 0 && m_main >= 2048) ? (int)m_main : 0;
}
static void tail_split_args(const ph_gemm_args& a, int m_main, ph_gemm_args& b, ph_gemm_args& c) {
  b = a; c = a;
  b.M = m_main;
  c.M = a.M - m_main;
  c.A = (const char*)a.A + (size_t)m_main * a.lda * 2;
  c.C = (char*)a.C + (size_t)m_main * a.ldc * (a.out_f32 ? 4 : 2);
  if (a.pre_out) c.pre_out = (char*)a.pre_out + (size_t)m_main * a.ldc * 2;
  if (a.act_in) c.act_in = (const char*)a.act_in + (size_t)m_main * a.ld_act * 2;
  if (a.residual) c.residual = (const char*)a.residual + (size_t)m_main * a.ldr * (a.residual_f32 ? 4 : 2);
}

static Route route_single(const ph_gemm_args& a, const Tuning& t) {
  Route r;
  if ((r.tail_m = tail_split_row(a)) > 0) return r;
  if ((a.conv && !a.trans_a && !a.trans_b) || a.a_colsum) {      // implicit-GEMM forward, fused column sums: the grouped kernels have them
    r = route_grouped(&a, 1, 0, t);
    r.as_group = true;
    return r;
  }
  r.ta = a.trans_a; r.tb = a.trans_b; r.start[0] = 0; r.nsplit[0] = 1;
  const BigVariant big = big_variant(t.big_mode);
  const int kt = ceil_div(a.K, BK);
  // ---- 256x128 LDS-DMA kernel: enough 256x128 tiles for the chip, and cheaper by block rounds than the 128x128 kernel (a tile count just
  // above a multiple of 256 favours the latter: 41 x 8 tiles of 256x128 are two full rounds, 81 x 8 of 128x128 one pair round + one lone round)
  const int64_t tbig = (int64_t)tiles_of(a, big::BM, big::BN);
  bool big_cheaper = true;
  if (t.big_min_tiles > 1) {
    const double ktd = (double)(a.K / BK);
    const int64_t t128b = (int64_t)tiles_of(a, 128, 128), rem = t128b % SLOTS128;
    const double cost_big = (double)ceil_div64(tbig, 256) * (ktd * fit::BIG_KTILE + fit::BIG_FIXED_SINGLE);
    const double cost_128 = (double)(t128b / SLOTS128) * (ktd * fit::PAIR128_KTILE + fit::R128_FIXED_SINGLE) +
                            (rem > 256 ? ktd * fit::PAIR128_KTILE + fit::R128_FIXED_SINGLE : (rem > 0 ? ktd * fit::LONE128_KTILE + fit::R128_FIXED_SINGLE : 0.0));
    big_cheaper = cost_big < cost_128 * (a.trans_b ? 1.0 : fit::NN_TIE);
  }
  const bool big_any = big != BigVariant::off && !a.conv && !a.col_stats && (a.K % BK) == 0 && a.split_k <= 0 && a.M >= big::BM && (a.N % 8) == 0 && a.N >= 8 && big_cheaper;
  // forward-shaped (B = [N][K]) and dgrad-shaped (B = [K][N]) problems: only the launches with N <= 1024 or a long k loop keep their isolated
  // gain inside the step (profiles/r2_ab_big_tile_gemm.txt, r2_gemm_by_grid.txt) -- the wide-N, K = 768 launches are write-out bound there
  const bool big_fwd = big_any && !a.trans_a && a.K >= 2 * BK && tbig >= t.big_min_tiles && (tbig >= 192 || a.K >= 32 * BK || t.big_min_tiles <= 1);
  // weight-gradient layout (A = [K][M], B = [K][N]) with a long reduction: same kernel, both operands through the transposing reads, ping-pong only
  const bool big_wgrad = big_any && a.trans_a && a.trans_b && a.K >= 32 * BK && (a.M % 8) == 0 && tbig >= 64;
  if (big_fwd || big_wgrad) {
    r.cls = PH_GEMM_CLS_BIG; r.bm = big::BM; r.bn = big::BN;
    r.variant = big_fwd ? big : (big == BigVariant::spread ? BigVariant::spread : BigVariant::lean);
    r.tiles_m[0] = ceil_div(a.M, big::BM); r.tiles_n[0] = ceil_div(a.N, big::BN); r.kt_per_split[0] = a.K / BK;
    r.start[1] = big_xcd_grid(r.tiles_m[0], r.tiles_n[0]);
    return r;
  }
  // ---- register-staged kernels: 128x128 tiles when they fill the chip; otherwise split the K loop (partials -> workspace -> fold pass with the
  // epilogue) so that >= ~2 blocks per CU are in flight; 64x64 tiles for genuinely small outputs.  (tile, split) by the fit::REG* model: waves of
  // co-resident blocks x (k-tiles x slope + fixed), a split adds the fold launch plus splits*M*N*4 bytes of partial traffic
  const int ldws = (a.N + 3) / 4 * 4;
  const bool plain_acc = plain_f32(a) && a.accumulate;
  auto ws_fits = [&](int sp) { return a.workspace && (int64_t)sp * a.M * ldws * 4 <= a.workspace_bytes; };
  const int64_t t128 = tiles_of(a, 128, 128), t64 = tiles_of(a, 64, 64);
  int BM = 128, splits = 1;
  if (a.split_k > 0) {
    splits = a.split_k;
    if (a.M <= 64 || a.N <= 64 || t128 * splits < 128) BM = 64;
  } else {
    double best = 1e30;
    const int cand[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256};   // (the stems' first-layer weight gradients:
                                                                                       //  2 output tiles, 6272 k-tiles -- 48 splits left them at 94 us)
    for (int bm = 64; bm <= 128; bm += 64) {
      if (bm == 128 && (a.M <= 64 || a.N <= 64)) continue;
      const double tiles = (double)(bm == 128 ? t128 : t64), cap = bm == 128 ? SLOTS128 : SLOTS64, t_iter = bm == 128 ? fit::REG128_KTILE : fit::REG64_KTILE;
      for (int sp : cand) {
        if (sp > 1 && (sp > kt / 2 || !(ws_fits(sp) || plain_acc))) continue;
        double cost = ceil(tiles * sp / cap) * (ceil((double)kt / sp) * t_iter + fit::REG_WAVE_FIXED);
        if (sp > 1) cost += fit::FOLD_LAUNCH + (double)sp * a.M * ldws * 4.0 / fit::FOLD_BYTES_PER_US;
        if (cost < best) { best = cost; BM = bm; splits = sp; }
      }
    }
  }
  if (splits > kt) splits = kt;
  // N = 64 mod 128 and narrow (the stems' N = 192 convs): 128x64 tiles cover N exactly instead of wasting half a column tile
  // (100352x192x864: 71 -> 66 us); on every other shape the narrower wave tile (one B fragment per two MFMAs) loses
  const int BN = (BM == 128 && splits == 1 && a.N % 128 == 64 && a.N <= 192) ? 64 : BM;
  r.cls = BM == 64 ? PH_GEMM_CLS_64 : PH_GEMM_CLS_128; r.bm = BM; r.bn = BN;
  r.tiles_m[0] = ceil_div(a.M, BM); r.tiles_n[0] = ceil_div(a.N, BN);
  // 64x64-tile launches that leave CUs with a single block (the decoder's M = 960 rows): split the k loop inside the block instead
  // of over gridDim.z + a fold launch.  also instead of a workspace split-K of a 64x64 launch
  if (BM == 64 && BN == 64 && !a.conv && !a.col_stats && !a.trans_a && (a.K % BK) == 0 && kt >= 8 && a.split_k <= 0 && t64 <= 512) {
    r.cls = PH_GEMM_CLS_KS2; r.kt_per_split[0] = kt;
    r.start[1] = r.tiles_m[0] * r.tiles_n[0];
    return r;
  }
  r.kt_per_split[0] = ceil_div(kt, splits);
  r.nsplit[0] = r.max_split = splits = ceil_div(kt, r.kt_per_split[0]);
  r.start[1] = r.tiles_m[0] * r.tiles_n[0] * splits;
  if (splits > 1 && ws_fits(splits)) {          // (without a workspace: plain fp32 accumulation with atomics, no fold pass)
    const bool wide = splits >= 32 && (int64_t)a.M * ((a.N + 3) / 4) <= 16384;       // many splits of a small output: 16 lanes per output vector
    r.fold = a.defer_reduce ? PH_GEMM_FOLD_DEFERRED : PH_GEMM_FOLD_PASS; r.fold_lanes = wide ? 16 : 1;
    r.ws_bytes = (size_t)splits * a.M * ldws * 4;
    r.ws_off[0] = 0;                            // (a deferred call: behind the partial sums already queued, run_single knows where)
  }
  return r;
}

// the arrival counters of a cut plan are zeroed by this kernel ahead of EVERY launch, on the launch's stream (a kernel, not a memset node:
// small memset nodes replay wrongly inside a captured step on this ROCm, see tests/test_abi.py)
__global__ void zero_counters_kernel(int* cnt, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = 0;
}

static int run_grouped(const ph_gemm_args* args, int n, int max_blocks, hipStream_t stream) {
  PH_CHECK_ARG(args && n >= 1 && n <= PH_GEMM_GROUP_MAX, "ph_gemm_grouped_bf16: need 1..%d problems, got %d", PH_GEMM_GROUP_MAX, n);
  double flops = 0.0, bytes = 0.0;
  for (int i = 0; i < n; ++i) {
    PH_CHECK_ARG(args[i].trans_a == args[0].trans_a && args[i].trans_b == args[0].trans_b, "ph_gemm_grouped_bf16: mixed layouts in one group");
    PH_CHECK_ARG((args[i].conv != nullptr) == (args[0].conv != nullptr), "ph_gemm_grouped_bf16: implicit-GEMM conv problems cannot share a group with plain ones");
    flops += 2.0 * args[i].M * (double)args[i].N * args[i].K;
    bytes += 2.0 * ((double)args[i].M * args[i].K + (double)args[i].N * args[i].K + (double)args[i].M * args[i].N);
  }
  char desc__[96];
  if (g_ph_prof_enabled) snprintf(desc__, sizeof(desc__), "gemm grouped n=%d ta=%d tb=%d K0=%d", n, args[0].trans_a, args[0].trans_b, args[0].K);
  ProfScope prof__(PH_FAM_GEMM, flops, bytes, stream, desc__);
  GroupParams g;                             // ~2.3 KB: copied into the kernel arguments by the launch
  g.n = n;
  for (int i = 0; i < n; ++i) {
    int rc = fill_params(&args[i], g.p[i]);
    if (rc) return rc;
  }
  const Route r = route_grouped(args, n, max_blocks, tuning_now(true));
  const bool big = r.cls == PH_GEMM_CLS_BIG_GROUPED;
  char* const ws = reinterpret_cast<char*>(args[0].workspace);
  for (int i = 0; i < n; ++i) {
    GemmParams& p = g.p[i];
    p.tiles_m = r.tiles_m[i]; p.tiles_n = r.tiles_n[i]; p.k_tiles_per_split = r.kt_per_split[i];
    g.nsplit[i] = r.nsplit[i]; g.tile_start[i] = r.start[i];
    p.ws = r.nsplit[i] > 1 ? reinterpret_cast<float*>(ws + r.ws_off[i]) : nullptr;
    p.tile_cnt = big && r.nsplit[i] > 1 ? reinterpret_cast<int*>(ws + r.cnt_off[i]) : nullptr;
    if (big && r.conv == 1) p.ldws = 0;
  }
  g.tile_start[n] = r.start[n];
  if (big && r.conv == 1) return big::launch_grouped_conv(g, r.start[n], r.variant, stream);
  if (big) {
    if (r.cnt_bytes > 0) {
      // zeroed on the stream ahead of EVERY launch (captured with the step): the counters of an earlier launch -- or of a launch that never
      // finished, or whatever the workspace held before -- are never trusted
      const int words = (int)(r.cnt_bytes / 4);
      hipLaunchKernelGGL(zero_counters_kernel, dim3(ceil_div(words, 256)), dim3(256), 0, stream, reinterpret_cast<int*>(ws), words);
      PH_LAUNCH_CHECK("zero_counters_kernel");
    }
    return big::launch_grouped_wgrad(g, r.start[n], r.variant, r.conv == 2, stream);
  }
  int rc = r.bm == 128 ? reg::launch_grouped_128(g, r.start[n], max_blocks, r.ta, r.tb, r.pf, r.conv, stream)
                       : reg::launch_grouped_64(g, r.start[n], max_blocks, r.ta, r.tb, r.pf, r.conv, stream);
  if (rc != PH_OK || r.fold == PH_GEMM_FOLD_NONE) return rc;
  ReduceGroup red;                           // ONE grouped pass folds the partial sums of the problems that were cut
  red.n = 0; red.blk_start[0] = 0;
  for (int i = 0; i < n; ++i) {
    if (r.nsplit[i] <= 1) continue;
    red.p[red.n] = g.p[i]; red.splits[red.n] = r.nsplit[i];
    red.blk_start[red.n + 1] = red.blk_start[red.n] + reduce_blocks(g.p[i], false);
    ++red.n;
  }
  count_launch(PH_GEMM_CLS_SPLITK_REDUCE);
  hipLaunchKernelGGL(splitk_reduce_grouped_kernel<1>, dim3(red.blk_start[red.n]), dim3(256), 0, stream, red);
  PH_LAUNCH_CHECK("splitk_reduce_grouped_kernel");
  return PH_OK;
}

extern "C" int ph_gemm_grouped_bf16(const ph_gemm_args* args, int n, hipStream_t stream) { return run_grouped(args, n, 0, stream); }
extern "C" int ph_gemm_grouped_capped_bf16(const ph_gemm_args* args, int n, int max_blocks, hipStream_t stream) {
  return run_grouped(args, n, max_blocks, stream);
}

extern "C" int ph_gemm_bf16(const ph_gemm_args* a, hipStream_t stream) {
  PH_CHECK_ARG(a && a->A && a->B && a->C, "ph_gemm_bf16: null pointer");
  PH_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "ph_gemm_bf16: bad dims M=%d N=%d K=%d", a->M, a->N, a->K);      // (the route divides by them)
  const Route r = route_single(*a, tuning_now(true));
  if (r.tail_m > 0) {       // (before the profiling scope of this call: the two halves are profiled as two launches)
    ph_gemm_args b, c;
    tail_split_args(*a, r.tail_m, b, c);
    int rc = ph_gemm_bf16(&b, stream);
    return rc != PH_OK ? rc : ph_gemm_bf16(&c, stream);
  }
  char desc__[96];
  if (g_ph_prof_enabled) snprintf(desc__, sizeof(desc__), "gemm M=%d N=%d K=%d ta=%d tb=%d f32=%d acc=%d", a->M, a->N, a->K, a->trans_a, a->trans_b, a->out_f32, a->accumulate);
  ProfScope prof__(PH_FAM_GEMM, 2.0 * a->M * (double)a->N * a->K, 2.0 * ((double)a->M * a->K + (double)a->N * a->K + (double)a->M * a->N), stream, desc__);
  if (r.as_group) return run_grouped(a, 1, 0, stream);
  GemmParams p;
  {
    int rc = fill_params(a, p);
    if (rc) return rc;
  }
  PH_CHECK_ARG(!a->col_stats || a->split_k <= 1, "ph_gemm_bf16: col_stats cannot be combined with split-K");
  const int splits = r.nsplit[0];
  p.tiles_m = r.tiles_m[0]; p.tiles_n = r.tiles_n[0]; p.k_tiles_per_split = r.kt_per_split[0];
  if (r.cls == PH_GEMM_CLS_BIG) {
    p.ldws = 0;
    return big::launch_single(p, r.variant, r.ta != 0, r.tb != 0, stream);
  }
  if (r.cls == PH_GEMM_CLS_KS2) return reg::launch_ks2(p, r.tb, stream);
  if (r.fold != PH_GEMM_FOLD_NONE) {
    p.ws = (float*)a->workspace;
    if (r.fold == PH_GEMM_FOLD_DEFERRED) {    // partial sums of consecutive deferred calls sit one after the other in the caller's workspace
      std::lock_guard<std::mutex> lock(g_defer_mu);
      const size_t need = (r.ws_bytes + 255) / 256 * 256;
      if (g_defer.empty()) g_defer_cursor = 0;
      if (!g_defer.empty() && (g_defer_ws != a->workspace || g_defer_cursor + need > (size_t)a->workspace_bytes)) {
        int rcf = flush_deferred_locked(stream);
        if (rcf != PH_OK) return rcf;
      }
      p.ws = reinterpret_cast<float*>(reinterpret_cast<char*>(a->workspace) + g_defer_cursor);
      g_defer_cursor += need;
      g_defer_ws = a->workspace;
    }
  } else PH_CHECK_ARG(splits <= 1 || (plain_f32(*a) && a->accumulate), "ph_gemm_bf16: split_k > 1 without workspace needs out_f32 + accumulate and no fused epilogue");
  int rc = r.bm == 64 ? reg::launch_single_64(p, r.ta, r.tb, splits, stream) : reg::launch_single_128(p, r.bn, r.ta, r.tb, splits, stream);
  if (rc != PH_OK || !p.ws) return rc;
  if (r.fold == PH_GEMM_FOLD_DEFERRED) {                  // the fold pass joins the queue (the partials stay where they are until the flush)
    std::lock_guard<std::mutex> lock(g_defer_mu);
    g_defer.push_back(DeferredReduce{p, splits, r.fold_lanes == 16});
    return PH_OK;
  }
  count_launch(PH_GEMM_CLS_SPLITK_REDUCE);
  if (r.fold_lanes == 16) hipLaunchKernelGGL(splitk_reduce_kernel<16>, dim3(reduce_blocks(p, true)), dim3(256), 0, stream, p, splits);
  else hipLaunchKernelGGL(splitk_reduce_kernel<1>, dim3(reduce_blocks(p, false)), dim3(256), 0, stream, p, splits);
  PH_LAUNCH_CHECK("splitk_reduce_kernel");
  return PH_OK;
}

extern "C" int ph_gemm_route(const ph_gemm_args* args, int n, int grouped, int max_blocks, ph_gemm_route_info* out) {
  PH_CHECK_ARG(args && out && n >= 1 && n <= (grouped ? PH_GEMM_GROUP_MAX : 1), "ph_gemm_route: need 1..%d problems and an output", grouped ? PH_GEMM_GROUP_MAX : 1);
  for (int i = 0; i < n; ++i) {
    PH_CHECK_ARG(args[i].M > 0 && args[i].N > 0 && args[i].K > 0, "ph_gemm_route: bad dims M=%d N=%d K=%d", args[i].M, args[i].N, args[i].K);
    PH_CHECK_ARG(args[i].trans_a == args[0].trans_a && args[i].trans_b == args[0].trans_b && (args[i].conv != nullptr) == (args[0].conv != nullptr) &&
                 (!args[i].conv || args[i].trans_a == args[i].trans_b), "ph_gemm_route: mixed layouts in one group, or a conv gather on a layout that has none");
  }
  const Tuning t = tuning_now(false);
  ph_gemm_args half[2];
  Route r = grouped ? route_grouped(args, n, max_blocks, t) : route_single(args[0], t);
  *out = ph_gemm_route_info{};
  out->parts = r.tail_m > 0 ? 2 : 1; out->tail_m = r.tail_m;
  if (r.tail_m > 0) tail_split_args(args[0], r.tail_m, half[0], half[1]);
  for (int k = 0; k < out->parts; ++k) {
    if (r.tail_m > 0 || k > 0) r = route_single(half[k], t);
    ph_gemm_route_part& o = out->part[k];
    o.cls = r.cls; o.bm = r.bm; o.bn = r.bn; o.variant = (int)r.variant; o.units = r.start[r.n]; o.max_split = r.max_split;
    o.fold = r.fold; o.fold_lanes = r.fold_lanes; o.ws_bytes = (int64_t)r.ws_bytes;
  }
  return PH_OK;
}
