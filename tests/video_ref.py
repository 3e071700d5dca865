"""numpy restatement of the video renderer's post-processing (R/luciddreamer.py:254-265), the contract of csrc/video.hip:
the frame expression, the depth value, np.percentile's float32 "linear" method spelled out, and colorize's normalisation and
colormap lookup with a given uint8 LUT (so that matplotlib is not needed).  tests/test_video_cpu.py checks it against the
reference's own output (tests/golden/ref_video_fixtures.npz); the GPU tests compare the kernels with it."""
import numpy as np

F = np.float32


def frame_u8(image):
    """image float32 [3,H,W] -> uint8 [H,W,3]."""
    x = np.ascontiguousarray(np.asarray(image, np.float32).transpose(1, 2, 0))
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, x, F(0))
        c = np.where(c < 1, c, F(1))
        return np.rint(c * F(255)).astype(np.uint8)


def depth_value(depth):
    """-(d * (d > 0)) in float32 as torch computes it, squeezed to [H,W]."""
    d = np.asarray(depth, np.float32).reshape(np.asarray(depth).shape[-2:])
    with np.errstate(invalid="ignore"):
        return -(d * (d > 0).astype(np.float32))


def percentile(vals, q):
    """numpy's float32 np.percentile(vals, q), "linear" method, restated: NaN if any value is NaN."""
    v = np.asarray(vals, np.float32).reshape(-1)
    n = v.size
    if n == 0:
        return F(np.nan)
    if np.isnan(v).any():
        return F(np.nan)
    s = np.sort(v)
    q32 = F(q) / F(100)
    vi = F(F(n - 1) * q32)
    lo = min(int(np.floor(vi)), n - 1)
    hi = min(lo + 1, n - 1)
    g = F(vi - F(lo))
    a, b = s[lo], s[hi]
    with np.errstate(invalid="ignore", over="ignore"):
        d = F(b - a)
        return F(b - d * (F(1) - g)) if g >= F(0.5) else F(a + d * g)


def colorize(value, lut, vmin=None, vmax=None, invalid_val=-99, background=(128, 128, 128, 255)):
    """R/utils/depth.py:colorize(value) with a uint8 [N+3, 4] LUT; value float32 [H,W].  Returns (rgba, vmin, vmax); a map
    without a valid pixel gives the background everywhere and NaN limits (the reference raises IndexError there)."""
    v = np.asarray(value, np.float32)
    invalid = v == F(invalid_val)
    valid = v[~invalid]
    vmin = percentile(valid, 2) if vmin is None else F(vmin)
    vmax = percentile(valid, 98) if vmax is None else F(vmax)
    N = lut.shape[0] - 3
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (v - vmin) / F(vmax - vmin) if vmin != vmax else v * F(0)
        x = (t * F(N)).astype(np.float32)
        x[x == F(N)] = F(N - 1)
        idx = np.zeros(x.shape, np.int64)
        ok = np.isfinite(x) & (x >= 0) & (x < N)
        idx[ok] = x[ok].astype(np.int64)
        idx[x < 0] = N
        idx[x >= N] = N + 1
        idx[np.isnan(x)] = N + 2
    rgba = lut[idx]
    rgba[invalid] = np.asarray(background, np.uint8)
    return rgba, vmin, vmax


# ---- the 512 x 512 fixture cases: inputs regenerated from a counter-based hash, outputs pinned by digest ----------------------
# A 512 x 512 case holds 4-7 MB of incompressible data; the fixture keeps only the SHA-256 of the reference's output bytes and
# its percentiles, and the inputs come from splitmix64 of the element index (integer arithmetic, then one exact float64 step
# rounded to float32): the same bits on every machine and numpy version.
def hash_uniform(seed, shape, lo, hi):
    """float32 array of `shape`, deterministic: lo + (hi - lo) * u with u = 24 hash bits / 2^24 in [0, 1)."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def big_depth_cases():
    """{name: float32 [1,512,512] rendered depth}: 97 % background, and a random map with a zero block."""
    d = hash_uniform(11, (1, 512, 512), 1.0, 20.0)
    d[hash_uniform(12, (1, 512, 512), 0.0, 1.0) >= 0.03] = 0.0
    r = hash_uniform(13, (1, 512, 512), 0.2, 30.0)
    r[0, 200:260, 100:400] = 0.0
    return {"bg97_512x512": d, "rand_512x512": r}


def frame_specials():
    """Frame values at the edges of the contract: every x whose float32 x * 255 is k + 0.5 (half-even ties), 1 - ulp, exact
    0 / 1 / -0, slightly and far below 0, above 1."""
    ties = []
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        for cand in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1))):
            if np.float32(cand) * np.float32(255.0) == np.float32(k + 0.5):
                ties.append(cand)
    assert len(ties) > 200, len(ties)
    return np.array(ties + [np.nextafter(np.float32(1), np.float32(0)), 0.0, 1.0, -0.0, -1e-8, -3.0, 1.0000001, 7.0],
                    np.float32)


def big_image_cases():
    """{name: float32 [3,512,512]}: uniform in [-0.2, 1.2) with frame_specials() at every 97th element."""
    special = frame_specials()
    x = hash_uniform(21, (3, 512, 512), -0.2, 1.2).reshape(-1)
    idx = np.arange(special.size) * 97
    x[idx] = special
    return {"rand_512x512": x.reshape(3, 512, 512)}


def digest(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
