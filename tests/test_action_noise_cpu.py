"""The action noise (include/sng.h, sng_noise_create; policy.ActionNoise) without a GPU, through sng_noise_host_fill and
a stand-alone g++ program over the header the kernel compiles (csrc/sng_noise_host.h):

  - the inverse CDF against float64 scipy.special.ndtri over every u < 65,536, 2^14 evenly spaced u in each of the 31
    octaves and 2^22 random hashes: max |z - ndtri(p)| <= 2^-18 (8 ulp of a float32 in [4, 8), where the tail lives);
    odd in the sign bit, never 0.  The figure measured on this build is printed (and recorded in DESIGN.md 4.6);
  - the law: KS of 2^22 Gaussian-kind variates against the normal law (an inverse-CDF error e moves the CDF by at most
    0.4 e, so this sees only gross faults), and the sample correlation between adjacent envs, actions, steps and
    counters, each within 5 / sqrt(n) of 0;
  - the stream: host_fill's variates are those of a numpy restatement of the key and the hash;
  - OU: host_fill equals a numpy float32 restatement of the recurrence on the Gaussian kind's z, bitwise, from 0 a day;
  - keys: shards equal the population, also above 2^32; four days equal two and two; another seed, counter or action
    changes every block;
  - every refusal gives its code and a message naming the value.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from smart_nanogrid_gym import _native, policy
from test_gpu_generator_distributions import P_MIN

special = pytest.importorskip("scipy.special")
stats = pytest.importorskip("scipy.stats")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smart-nanogrid-gym_amd", "csrc")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
SOURCE = os.path.join(ROOT, "tests", "native", "noise_host_check.cpp")
BOUND = 2.0 ** -18

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """variates(h uint32 array) -> float32 array, by the stand-alone program built from the header with plain g++."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("noise_native")
    exe = str(tmp / "noise_host_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O2", *INCLUDES, SOURCE, "-o", exe],
                   check=True)

    def variates(h):
        h = np.ascontiguousarray(h, dtype=np.uint32)
        fin, fout = str(tmp / "h.u32"), str(tmp / "z.f32")
        h.tofile(fin)
        out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "noise host ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        assert int(out.stdout.split()[-2]) == h.size
        return np.fromfile(fout, dtype=np.float32)
    variates.exe = exe
    return variates


@needs_gxx
def test_host_header_self_checks(native):
    out = subprocess.run([native.exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "noise host ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@needs_gxx
def test_host_header_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined, run directly."""
    exe = str(tmp_path / "noise_host_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INCLUDES, SOURCE, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "noise host ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def _want(h):
    """float64 ndtri of the hash's p, with the sign bit's sign: z = sign ? ndtri(p) : -ndtri(p)."""
    u = np.maximum(h & np.uint32(0x7fffffff), np.uint32(1)).astype(np.float64)
    q = special.ndtri((u + 0.5) * 2.0 ** -32)
    return np.where(h >> np.uint32(31), q, -q)


def test_inverse_cdf_against_ndtri(native):
    rng = np.random.default_rng(20260)
    sets = {"u < 65536": np.arange(65536, dtype=np.uint32),
            "2^22 random h": rng.integers(0, 2 ** 32, 1 << 22, dtype=np.uint64).astype(np.uint32)}
    for k in range(31):
        lo = 1 << (30 - k)
        sets[f"octave {k}"] = np.unique((lo + np.arange(1 << 14) * (lo / float(1 << 14))).astype(np.uint32))
    worst, zmax = 0.0, 0.0
    for name, u in sets.items():
        hs = [u] if name.startswith("2^22") else [u, u | np.uint32(0x80000000)]
        zs = [native(h) for h in hs]
        for h, z in zip(hs, zs):
            assert np.all(z != 0) and np.all(np.isfinite(z)), name
            err = float(np.max(np.abs(z.astype(np.float64) - _want(h))))
            assert err <= BOUND, (name, err)
            worst, zmax = max(worst, err), max(zmax, float(np.max(np.abs(z))))
        if len(zs) == 2:   # odd in the sign bit
            assert np.array_equal(zs[1], -zs[0]) and np.all(zs[0] > 0), name
    print(f"inverse CDF: max |z - ndtri(p)| = {worst:.3e} (bound {BOUND:.3e}), max |z| = {zmax:.4f}")
    assert zmax <= 6.17


# ---- through sng_noise_host_fill ----
E_LAW, A_LAW, T_LAW, DAYS_LAW = 64, 8, 32, 256   # 2^22 variates


@pytest.fixture(scope="module")
def law():
    z = policy.noise_host_fill("gaussian", A_LAW, T_LAW, E_LAW, days=DAYS_LAW, seed=77, mu=0.0, scale=1.0, counter=5)
    assert z.shape == (DAYS_LAW, T_LAW, E_LAW, A_LAW) and z.size == 1 << 22
    z.setflags(write=False)
    return z


def test_gaussian_law(law):
    p = stats.kstest(law.reshape(-1).astype(np.float64), "norm")[1]
    print(f"KS p = {p:.3g} at n = 2^22, mean {law.mean():.2e}, std {law.std():.6f}")
    assert p > P_MIN


def test_no_correlation_between_neighbours(law):
    z = law.astype(np.float64)

    def corr(a, b):
        a, b = a.reshape(-1), b.reshape(-1)
        return float(np.corrcoef(a, b)[0, 1]), a.size
    pairs = {"envs": (z[:, :, :-1], z[:, :, 1:]), "actions": (z[..., :-1], z[..., 1:]),
             "steps": (z[:, :-1], z[:, 1:]), "counters": (z[:-1], z[1:])}
    for name, (a, b) in pairs.items():
        r, n = corr(a, b)
        print(f"correlation of adjacent {name}: {r:+.2e} (n = {n}, bound {5 / np.sqrt(n):.2e})")
        assert abs(r) <= 5 / np.sqrt(n), name


def _mix32(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(17)
    x = (x * np.uint64(0xed5ad4bb)) & m
    x ^= x >> np.uint64(11)
    x = (x * np.uint64(0xac4c1b51)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x31848bab)) & m
    x ^= x >> np.uint64(14)
    return x


def _hashes(seed, ge, j, c, T):
    """include/sng.h's stream, restated: h [len(ge), len(j), T] of (seed, ge, j, c)."""
    m, u = np.uint64(0xffffffff), np.uint64
    one = lambda v: np.array([v], dtype=np.uint64)   # noqa: E731
    k0 = _mix32(one(seed & 0xffffffff) ^ _mix32(one(((seed >> 32) + (c & 0xffffffff) * 0x9e3779b9) & 0xffffffff)))
    dk = _mix32(k0 ^ one(((c >> 32) * 0x85ebca6b + 0x165667b1) & 0xffffffff))
    ge = np.asarray(ge, dtype=np.uint64)[:, None]
    j = np.asarray(j, dtype=np.uint64)[None, :]
    k1 = _mix32(dk ^ (ge & m))
    lane = (((ge >> u(32)) * u(0x85ebca6b)) & m) + (((u(0x6e7a0000) | j) * u(0xc2b2ae35)) & m) + u(0x27d4eb2f)
    key = _mix32(k1 ^ (lane & m))
    t = np.arange(T, dtype=np.uint64)[None, None, :]
    return _mix32((key[:, :, None] + t * u(0x9e3779b9)) & m).astype(np.uint32)


@pytest.mark.parametrize("seed, offset, counter", [(3, 0, 0), (2 ** 40 + 9, 2 ** 33 + 5, 2 ** 35 + 1)])
def test_stream_is_the_documented_key_and_hash(native, seed, offset, counter):
    E, A, T = 7, 5, 6
    z = policy.noise_host_fill("gaussian", A, T, E, days=2, seed=seed, env_offset=offset, counter=counter)
    for d in range(2):
        h = _hashes(seed, offset + np.arange(E), np.arange(A), counter + d, T)   # [E, A, T]
        want = native(h.reshape(-1)).reshape(E, A, T).transpose(2, 0, 1)
        assert np.array_equal(z[d].view(np.uint32), want.view(np.uint32))


def test_gaussian_kind_is_mu_plus_scale_z():
    mu = np.array([0.5, -2.0, 0.0], np.float32)
    scale = np.array([0.3, 1.7, 0.0], np.float32)
    z = policy.noise_host_fill("gaussian", 3, 4, 9, days=2, seed=1)
    n = policy.noise_host_fill("gaussian", 3, 4, 9, days=2, seed=1, mu=mu, scale=scale)
    assert np.array_equal(n.view(np.uint32), (mu + scale * z).astype(np.float32).view(np.uint32))
    assert np.all(n[..., 2] == 0)


@pytest.mark.parametrize("theta, dt", [(0.15, 1e-2), (0.7, 0.25)])
def test_ou_is_the_recurrence_on_the_gaussian_variates(theta, dt):
    E, A, T, days = 11, 4, 24, 3
    mu = np.array([0.0, 0.4, -1.0, 2.0], np.float32)
    scale = np.array([0.5, 0.2, 1.5, 0.0], np.float32)
    kw = dict(seed=99, env_offset=17, counter=1000)
    z = policy.noise_host_fill("gaussian", A, T, E, days=days, **kw)
    ou = policy.noise_host_fill("ou", A, T, E, days=days, mu=mu, scale=scale, theta=theta, dt=dt, **kw)
    th, dtf = np.float32(theta), np.float32(dt)
    sd = (scale.astype(np.float64) * np.sqrt(np.float64(dt))).astype(np.float32)
    want = np.zeros_like(ou)
    for d in range(days):
        x = np.zeros((E, A), np.float32)   # every day starts from 0
        for t in range(T):
            x = ((x + ((th * (mu - x)) * dtf)).astype(np.float32) + (sd * z[d, t]).astype(np.float32)).astype(np.float32)
            want[d, t] = x
    assert want.dtype == np.float32 and np.array_equal(ou.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ou[:, 0].view(np.uint32),
                          ((th * mu) * dtf + (sd * z[:, 0]).astype(np.float32)).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("kind", ["gaussian", "ou"])
@pytest.mark.parametrize("base", [0, 2 ** 32 + 11])
def test_shards_equal_the_population(kind, base):
    E, A, T = 200, 3, 5
    kw = dict(days=2, seed=4, mu=0.1, scale=0.7, counter=3)
    whole = policy.noise_host_fill(kind, A, T, E, env_offset=base, **kw)
    a = policy.noise_host_fill(kind, A, T, 70, env_offset=base, **kw)
    b = policy.noise_host_fill(kind, A, T, 130, env_offset=base + 70, **kw)
    assert np.array_equal(np.concatenate([a, b], axis=2).view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("kind", ["gaussian", "ou"])
def test_four_days_are_two_and_two(kind):
    kw = dict(seed=8, mu=0.0, scale=1.0)
    c = 2 ** 32 - 1   # the second pair's counters are above 2^32
    four = policy.noise_host_fill(kind, 2, 6, 10, days=4, counter=c, **kw)
    two = [policy.noise_host_fill(kind, 2, 6, 10, days=2, counter=c + k, **kw) for k in (0, 2)]
    assert np.array_equal(four.view(np.uint32), np.concatenate(two).view(np.uint32))


def test_seed_counter_and_action_change_every_block():
    kw = dict(days=3, mu=0.0, scale=1.0)
    base = policy.noise_host_fill("gaussian", 4, 8, 32, seed=5, counter=10, **kw)
    others = {"seed": policy.noise_host_fill("gaussian", 4, 8, 32, seed=6, counter=10, **kw),
              "seed high word": policy.noise_host_fill("gaussian", 4, 8, 32, seed=5 + 2 ** 32, counter=10, **kw),
              "counter": policy.noise_host_fill("gaussian", 4, 8, 32, seed=5, counter=13, **kw),
              "counter high word": policy.noise_host_fill("gaussian", 4, 8, 32, seed=5, counter=10 + 2 ** 32, **kw),
              "env high word": policy.noise_host_fill("gaussian", 4, 8, 32, seed=5, counter=10, env_offset=2 ** 32, **kw)}
    for name, other in others.items():
        for d in range(3):   # 1,024 variates a block: equal ones are chance
            assert np.mean(other[d] == base[d]) < 0.01, (name, d)
    assert np.array_equal(base[1:], policy.noise_host_fill("gaussian", 4, 8, 32, seed=5, counter=11, days=2, mu=0.0, scale=1.0))
    for d in range(3):
        for j in range(3):
            assert np.mean(base[d, ..., j] == base[d, ..., j + 1]) < 0.01, (d, j)


def _rc(spec=None, mu="ok", scale="ok", T=4, E=3, days=2, out="ok", **spec_fields):
    f = dict(kind=1, act_dim=3, seed=0, theta=0.15, dt=1e-2)
    f.update(spec_fields)
    s = _native.SngNoiseSpec(f["kind"], f["act_dim"], f["seed"], f["theta"], f["dt"])
    A = max(1, min(f["act_dim"], 300))
    F = _native.c_float_p
    arr = lambda v, fill: (None if v is None else   # noqa: E731
                           (np.full(A, fill, np.float32) if isinstance(v, str) else np.asarray(v, np.float32)))
    mu, scale = arr(mu, 0.0), arr(scale, 1.0)
    buf = np.zeros(max(days, 1) * max(T, 1) * max(E, 1) * A, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(F)   # noqa: E731
    rc = _native.lib().sng_noise_host_fill(None if spec == "null" else ctypes.byref(s), ptr(mu), ptr(scale), T, E, 0, 0,
                                           days, None if out is None else ptr(buf))
    return rc, (_native.lib().sng_last_error(None) or b"").decode()


def test_refusals_name_the_value():
    assert _rc()[0] == 0 and _rc(mu=None)[0] == 0 and _rc(kind=0)[0] == 0
    for a in (0, -3, 256):
        rc, msg = _rc(act_dim=a)
        assert rc == -1 and str(a) in msg and "act_dim" in msg, msg
    assert _rc(act_dim=255)[0] == 0
    rc, msg = _rc(kind=7)
    assert rc == -1 and "kind 7" in msg
    for field in ("theta", "dt"):
        for bad in (float("inf"), float("nan")):
            rc, msg = _rc(**{field: bad})
            assert rc == -1 and field in msg and str(bad) in msg, msg
            assert _rc(kind=0, **{field: bad})[0] == -1
    rc, msg = _rc(dt=-0.5)
    assert rc == -1 and "dt" in msg and "negative" in msg
    for name in ("mu", "scale"):
        for bad in (float("inf"), float("nan")):
            rc, msg = _rc(**{name: [0.5, bad, 0.5]})
            assert rc == -1 and f"{name}[1]" in msg and str(bad) in msg, msg
    rc, msg = _rc(scale=[1.0, 1.0, -0.25])
    assert rc == -1 and "scale[2]" in msg and "-0.25" in msg and "negative" in msg
    rc, msg = _rc(days=0)
    assert rc == -1 and "days = 0" in msg
    rc, msg = _rc(days=-2)
    assert rc == -1 and "days = -2" in msg
    assert _rc(T=0)[0] == -1 and _rc(E=0)[0] == -1
    for null in (dict(spec="null"), dict(scale=None), dict(out=None)):
        rc, msg = _rc(**null)
        assert rc == -1 and "null" in msg, msg
    # the Python layer surfaces the code, and names its own refusals
    with pytest.raises(_native.NativeError, match="libsng error -1.*scale"):
        policy.noise_host_fill("ou", 3, 4, 3, scale=-1.0)
    with pytest.raises(ValueError, match="kind must be one of"):
        policy.noise_host_fill("uniform", 3, 4, 3)
    with pytest.raises(ValueError, match="scale must be a scalar or have shape"):
        policy.noise_host_fill("ou", 3, 4, 3, scale=[1.0, 2.0])


def test_the_committed_table_is_what_the_fitting_script_gives():
    """tools/fit_noise_table.py's output is the initialiser in csrc/sng_noise_host.h, value for value."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("fit_noise_table", os.path.join(ROOT, "tools", "fit_noise_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = open(os.path.join(CSRC, "sng_noise_host.h")).read()
    body = src[src.index("kNoiseIcdf[kNoiseOctaves * kNoiseSubs * 4] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    vals = np.array([float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", body)], np.float32)
    assert vals.size == 31 * 4 * 4
    fit = mod.fit().reshape(-1)
    # the fit is a float64 least-squares solve: another LAPACK may move a coefficient by an ulp
    assert np.allclose(vals, fit, rtol=3e-7, atol=0), int(np.argmax(np.abs(vals - fit)))
