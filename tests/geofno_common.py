"""Shared by tests/golden/make_geofno_golden.py and tests/test_geofno*.py: the FNO1d cases of the fixture and the stated draw of
their parameters (the `yaml` model has 2.6 M spectral weights, so the fixture stores no parameter values: both sides draw them
from the case's seed, as float32-representable numbers)."""
import numpy as np

CASES = {
    "yaml": dict(kw=dict(modes=64, width=64, padding=100, output_np=2001), B=2, s=2001, seed=21),
    "odd": dict(kw=dict(modes=6, width=8, padding=5, output_np=29), B=3, s=37, seed=22),
    "nyq": dict(kw=dict(modes=21, width=8, padding=8, output_np=40), B=2, s=40, seed=23),
    "trunc": dict(kw=dict(modes=6, width=8, padding=5, output_np=8), B=3, s=37, seed=24),
}
SAMPLE = 2000  # entries of each large gradient tensor of the `yaml` case kept in the fixture


def draw_params(names_shapes, width, seed):
    """{name: float64 array of float32-representable values}, drawn in the order given.  Spectral weights U(0, 1 / width): as
    strong a path as the 1x1 convolution beside it; biases N(0, 0.1); 1x1 convolutions N(0, 1 / in); linear layers Glorot."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in names_shapes:
        shp = tuple(int(v) for v in shp)
        if "weights1" in name:
            v = rng.uniform(0.0, 1.0 / width, shp)
        elif name.endswith("bias"):
            v = rng.normal(0.0, 0.1, shp)
        elif name.startswith("w"):
            v = rng.normal(0.0, np.sqrt(1.0 / shp[1]), shp)
        else:
            v = rng.normal(0.0, np.sqrt(2.0 / (shp[0] + shp[1])), shp)
        out[name] = np.asarray(v).astype(np.float32).astype(np.float64)
    return out


def draw_inputs(case):
    """(x [B, s, 2] float32: a smooth curve per sample and its abscissa, the cotangent w [B, output_np, 1] float64)."""
    c = CASES[case]
    rng = np.random.default_rng(1000 + c["seed"])
    t = np.linspace(0, 1, c["s"])
    amp, ph, k = rng.uniform(0.5, 1.5, (c["B"], 1)), rng.uniform(0, np.pi, (c["B"], 1)), rng.integers(1, 4, (c["B"], 1))
    curve = amp * np.sin(2 * np.pi * k * t[None] + ph) + 0.1 * rng.standard_normal((c["B"], c["s"]))
    x = np.stack([curve, np.broadcast_to(t[None], curve.shape)], -1).astype(np.float32)
    w = rng.standard_normal((c["B"], c["kw"]["output_np"], 1))
    return x, w


def sample_index(name, size):
    """The fixed index sample of a large gradient tensor (flattened)."""
    rng = np.random.default_rng(abs(hash_name(name)))
    return np.sort(rng.choice(size, size=min(SAMPLE, size), replace=False))


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (1 << 31)
    return h
