"""General pinhole cameras and exact-zero image regions for the parity tests.

synth.make_inputs draws one family of intrinsics -- [[fx,0,cx],[0,fy,cy],[0,0,1]], scale s = scale 0 over 2**s -- and keeps every
image value away from exactly 0.  The C ABI accepts ANY invertible 3x3 per (sample, scale) and the reference masks a warped pixel
whose three channels are exactly 0 (models/base_model.py:96), so the tests need inputs that the generator (shared with bench.py, hence
left alone) does not make.  Test infrastructure only; NumPy on the host."""
import numpy as np

KINDS = ("skew", "bottom", "per_scale", "scaled", "general")


# Largest |K[2,0]|, |K[2,1]| at scale 0.  Twice the 1.5e-3 first measured, and every draw at least half of it: with draws near 0
# (two samples: likely) the explainability mode, whose d_disp is mostly the smoothness term, moved by less than ten tolerances when
# K20 or K21 was ignored (tests/test_oracle_vs_torch_cpu.py prints the factor of every case).
BOTTOM_AMP = 3e-3


def cameras(d, kind, seed):
    """A new (B,S,3,3) float32 array made from d["intrinsics"]:
      skew       K[0,1] = fx U(-0.05, 0.05), K[1,0] = fy U(-0.03, 0.03), one draw per sample (fx, fy: that scale's)
      bottom     K[2,0], K[2,1] = +-U(0.5, 1) BOTTOM_AMP 2**s, K[2,2] = U(0.8, 1.25), one draw per sample
      per_scale  rows 0-1 of every (sample, scale) times their own U(0.97, 1.03): scale s is no longer scale 0 over 2**s
      scaled     the whole matrix times U(2, 5), one draw per sample
      general    skew, bottom and per_scale together"""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (KINDS, kind))
    K = np.array(d["intrinsics"], dtype=np.float64)
    B, S = K.shape[:2]
    rng = np.random.RandomState(seed)
    if kind in ("skew", "general"):
        a, c = rng.uniform(-0.05, 0.05, B), rng.uniform(-0.03, 0.03, B)
        K[:, :, 0, 1] = K[:, :, 0, 0] * a[:, None]
        K[:, :, 1, 0] = K[:, :, 1, 1] * c[:, None]
    if kind in ("bottom", "general"):
        p = BOTTOM_AMP * rng.uniform(0.5, 1.0, (B, 2)) * rng.choice([-1.0, 1.0], (B, 2))
        K[:, :, 2, :2] = p[:, None, :] * (2.0 ** np.arange(S))[None, :, None]
        K[:, :, 2, 2] = rng.uniform(0.8, 1.25, B)[:, None]
    if kind in ("per_scale", "general"):
        K[:, :, :2, :] *= rng.uniform(0.97, 1.03, (B, S, 2, 1))
    if kind == "scaled":
        K *= rng.uniform(2.0, 5.0, B)[:, None, None, None]
    return np.ascontiguousarray(K, dtype=np.float32)


def with_cameras(d, kind, seed):
    """d with its intrinsics replaced (kind None: d itself)"""
    return d if kind is None else dict(d, intrinsics=cameras(d, kind, seed))


# What a kernel that took a shortcut through K would compute: the same inputs with that shortcut applied to K.  A test on the camera
# `kind` can only notice the shortcuts listed for it (the others leave that K unchanged) -- tests/test_oracle_vs_torch_cpu.py checks
# both halves of this table and that every listed shortcut moves a compared quantity by ten times its tolerance.
def _entry(i, j, v):
    def f(K):
        K = K.copy()
        K[:, :, i, j] = v
        return K
    return f


def _rebuilt_from_scale_0(K):
    """every scale as multi_scale_intrinsics would derive it from scale 0 (rows 0-1 over 2**s; a bottom row follows the pixel
    coordinates the other way)"""
    out = np.repeat(K[:, :1], K.shape[1], axis=1)
    for s in range(K.shape[1]):
        f = np.float32(2 ** s)
        out[:, s, :2, :] /= f
        out[:, s, 2, :2] *= f
    return out


ABLATIONS = {
    "K01=0": _entry(0, 1, 0.0),
    "K10=0": _entry(1, 0, 0.0),
    "K20=0": _entry(2, 0, 0.0),
    "K21=0": _entry(2, 1, 0.0),
    "K22=1": _entry(2, 2, 1.0),
    "scales rebuilt from scale 0": _rebuilt_from_scale_0,
    "K/K22": lambda K: (K / K[:, :, 2:3, 2:3]).astype(np.float32),
}
ABLATIONS_OF = {
    "skew": ("K01=0", "K10=0"),
    "bottom": ("K20=0", "K21=0", "K22=1", "K/K22"),
    "per_scale": ("scales rebuilt from scale 0",),
    "scaled": ("K22=1", "K/K22"),
    "general": tuple(ABLATIONS),
}


def zero_regions(d):
    """A copy of d whose pyramids hold exact zeros, per scale (h, w that scale's size):
      * all three channels of the target and of every source are 0 in rows h//4 .. h//4 + max(h//3, 3), columns w//3 .. w//3 +
        max(w//4, 4): samples that land inside are IN VIEW and masked (models/base_model.py:96);
      * channel 1 of every source is 0 over the bottom quarter and left half, channel 2 of the target over the top fifth and right
        half: one zero channel does not mask a pixel.
    Returns (d', rect, one_src, one_tgt): the three regions as (h,w) bool arrays per scale."""
    tgt = [a.copy() for a in d["tgt_pyr"]]
    src = [a.copy() for a in d["src_pyr"]]
    rect, one_src, one_tgt = [], [], []
    for s in range(len(tgt)):
        h, w = tgt[s].shape[2:]
        r = np.zeros((h, w), bool)
        r[h // 4:h // 4 + max(h // 3, 3), w // 3:w // 3 + max(w // 4, 4)] = True
        a = np.zeros((h, w), bool)
        a[h - h // 4:, :w // 2] = True
        b = np.zeros((h, w), bool)
        b[:h // 5, w - w // 2:] = True
        tgt[s][:, :, r] = 0
        src[s][:, :, r] = 0
        src[s][:, 1::3][:, :, a] = 0
        tgt[s][:, 2][:, b] = 0
        rect.append(r), one_src.append(a), one_tgt.append(b)
    return dict(d, tgt_pyr=tgt, src_pyr=src), rect, one_src, one_tgt


# The shapes (B, H, W, n_src, n_scales) of tests/test_cameras_gpu.py with the seed of each: strips and partial strips, two and three
# scales, two and four sources, and a batch of 9 (a remainder when samples are dealt over the 8 XCDs).  The CPU test that shows
# the ablations above to be visible (tests/test_oracle_vs_torch_cpu.py) runs on exactly these inputs.
CASES = {(2, 32, 48, 2, 3): 31, (3, 20, 130, 4, 2): 11, (9, 16, 24, 2, 2): 7}
# the loss mode each single kind runs in (the general kind runs in all four)
MODES = ("l1", "ssim_smooth", "edge_aware", "explain")
MODE_OF = {"skew": "ssim_smooth", "bottom": "explain", "per_scale": "edge_aware", "scaled": "l1"}


def camera_inputs(synth, shape, kind, zeros=False):
    """The inputs of one camera case: synth's for the shape's seed (explainability logits included), the cameras of `kind` (None:
    synth's own) drawn with a seed of their own, optionally with the exact-zero regions."""
    B, H, W, n_src, n_scales = shape
    seed = CASES[tuple(shape)]
    d = with_cameras(synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=seed, with_masks=True), kind, 1000 + seed)
    return zero_regions(d)[0] if zeros else d
