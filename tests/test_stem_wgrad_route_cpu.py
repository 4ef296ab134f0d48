"""CPU: where ph_gemm_route sends the headline's (Prismer-BASE caption, batch 32) per-layer groups of stem conv weight gradients -- one
group per layer, the six experts' [K][M] x [K][N] problems with B gathered from the NHWC activation, sharing one workspace -- and that a
group the persistent 256x128 kernel cannot take keeps its earlier route.  Shapes as in tests/golden/gemm_routes.json (the single-call
rows of base_b32).  The numbers are the plan of prismer_amd/csrc/gemm.hip (plan_big_wgrad, fit:: constants): a changed constant is a
diff of this file."""
import ctypes as C

from prismer_amd import _lib

WS = 256 << 20

# (Cout, (B, H, W, C, ks, stride)) x experts: three dense stems (stride 2 throughout) and three label stems (strides 2, 2, 1, 1)
LAYER4 = [(768, (32, 28, 28, 384, 3, 2))] * 3 + [(768, (32, 14, 14, 384, 3, 1))] * 3            # 6 x (768, 3456, 6272)
LAYER3 = [(384, (32, 56, 56, 192, 3, 2))] * 3 + [(384, (32, 14, 14, 192, 3, 1))] * 3            # 3 x (384, 1728, 25088) + 3 x (384, 1728, 6272)
LAYER2 = [(192, (32, 112, 112, 96, 3, 2))] * 3 + [(192, (32, 28, 28, 96, 3, 2))] * 3            # 3 x (192, 864, 100352) + 3 x (192, 864, 6272)
LAYER1_LABEL = [(96, (32, 56, 56, 64, 3, 2))] * 3                                               # 3 x (96, 576, 25088)


def group(spec, ws=WS):
    arr, keep = (_lib.GemmArgs * len(spec))(), []
    for g, (Co, cv) in zip(arr, spec):
        B, H, W, Cc, ks, stride = cv
        Ho = (H + 2 * (ks // 2) - ks) // stride + 1
        g.A, g.B, g.C = 4096, 4096, 4096                      # (the route looks at presence and alignment only)
        g.M, g.N, g.K = Co, ks * ks * Cc, B * Ho * Ho
        g.lda, g.ldb, g.ldc = Co, g.N, g.N
        g.trans_a, g.trans_b, g.out_f32, g.alpha = 1, 1, 1, 1.0
        cg = _lib.ConvGather(*cv)
        keep.append(cg)
        g.conv = C.pointer(cg)
        if ws:
            g.workspace, g.workspace_bytes = 8192, ws
    return arr, keep


def route(spec, ws=WS):
    arr, keep = group(spec, ws)
    info = _lib.GemmRouteInfo()
    _lib.check(_lib.lib.ph_gemm_route(arr, len(spec), 1, 0, C.byref(info)), 'ph_gemm_route')
    assert info.parts == 1
    r = info.part[0]
    return dict(cls=_lib.GEMM_CLS[r.cls], tile=(r.bm, r.bn), units=r.units, cut=r.max_split, fold=r.fold, ws=r.ws_bytes)


SLAB = 256 * 128 * 4


def test_layer4_runs_whole_in_two_rounds():
    """486 tiles of 98 k-tiles: 256 + 230, no cut that the 21-k-tile floor and the slab cost allow fills the rounds better"""
    assert route(LAYER4) == dict(cls='big_grouped', tile=(256, 128), units=486, cut=1, fold=_lib.GEMM_FOLD_NONE, ws=0)
    assert route(LAYER4, ws=0) == route(LAYER4)


def test_layer3_is_cut_and_folded_in_the_launch():
    """2 x 14 tiles per problem (M = 384 pads to two row tiles); the dense problems (392 k-tiles) are cut, the label ones (98) stay whole"""
    r = route(LAYER3)
    assert (r['cls'], r['tile'], r['fold']) == ('big_grouped', (256, 128), _lib.GEMM_FOLD_IN_LAUNCH), r
    assert (r['units'], r['cut']) == LAYER3_PLAN, r
    dense_tiles = 3 * 28
    assert r['ws'] == 3 * 256 + dense_tiles * r['cut'] * SLAB, r            # one 256-B counter block per cut problem + its slabs
    # no workspace, nothing can be cut: 168 whole tiles of up to 392 k-tiles on 256 blocks model slower than the 252 tiles of the 128x128
    # grid (two per CU), which is also what the group got before
    without = route(LAYER3, ws=0)
    assert (without['cls'], without['tile'], without['units'], without['cut'], without['fold']) == ('grouped', (128, 128), 252, 1, _lib.GEMM_FOLD_NONE), without


def test_layer2_goes_by_cost_not_by_rule_order():
    """M = 192 covers no whole 256-row tile, so the rule order alone would hand the group to the register-staged k split; the modelled
    costs put it on the persistent units"""
    r = route(LAYER2)
    assert (r['cls'], r['tile'], r['fold']) == ('big_grouped', (256, 128), _lib.GEMM_FOLD_IN_LAUNCH), r
    assert (r['units'], r['cut']) == LAYER2_PLAN, r


def test_layer1_label_stays_on_the_register_staged_split():
    """3 x (96, 576, 25088): 15 tiles of 256x128, 63 % of them padding (M = 96 of 256 rows, N = 576 of 640 columns).  Cut to the floor the
    persistent plan models at ~37 us against ~34 us for the 64x64 register-staged k split + fold pass, so the group keeps the latter --
    and stems_bwd, which groups only what the persistent kernel takes, keeps the per-expert calls for this layer."""
    r = route(LAYER1_LABEL)
    assert (r['cls'], r['tile'], r['fold']) == ('grouped', (64, 64), _lib.GEMM_FOLD_PASS), r


def test_groups_the_persistent_kernel_cannot_take_keep_their_route():
    # one reduction that is no multiple of 64 pixels (31 x 14 x 14 = 6076)
    odd = LAYER4[:5] + [(768, (31, 14, 14, 384, 3, 1))]
    before = dict(cls='grouped', tile=(128, 128), units=972, cut=1, fold=_lib.GEMM_FOLD_NONE, ws=0)
    assert route(odd) == before
    # the 256x128 kernels switched off
    _lib.lib.ph_gemm_tuning(0, -1)
    try:
        assert route(LAYER4) == before
        assert route(LAYER3)['cls'] == 'grouped' and route(LAYER2)['cls'] == 'grouped'
    finally:
        _lib.lib.ph_gemm_tuning(*_lib.GEMM_BIG_DEFAULT)
    # fewer than 32 k-tiles (the hand row of the golden table: K = 256)
    assert route([(128, (1, 16, 16, 64, 3, 1))], ws=0) == dict(cls='grouped', tile=(64, 64), units=18, cut=1, fold=_lib.GEMM_FOLD_NONE, ws=0)


LAYER3_PLAN = (504, 5)
LAYER2_PLAN = (252, 11)
