"""ismpc_a_tick_batch_horizon_device: the tick with its whole decision `dec` and predicted horizon `pred`, on the ticks
of the exact fixtures tests/golden/formA_exact_*.npz -- C in {65, 100, 160, 200} and the edges group's {5, 65, 129, 193, 250, 253}, F = 3 .. 6,
batches of 16 to 92 instances (32 to 184 lanes of the prediction kernel: across wavefront and tile boundaries) and batch 1.

Every call gets dec and pred filled with a sentinel bit pattern and 64 guard doubles behind each: afterwards no sentinel is left inside
and the guards are intact.

  SAME TICK      state and out bytes (and, in fp32, the deferred count) equal the plain tick's, in every form: wave, block, cold, hist,
                 per-instance with ISMPC_A_BUCKET 0 | 1, fp32 with ISMPC_A_F32_RESOLVE on | off, and a caller-driven warm-history loop.
  DECISION fp64  over the sol_idx ticks u within 16 x floor_u of the exact sol[:C] and f within 16 x floor_f of sol[C:C+F]
                 (tests/golden/formA_horizon_floors.npz: reference-side floors, 16 = exact_tick_a.BOUND_FACTOR); dec[.., 0] and dec[.., C]
                 are out.u0 / out.f0 by bytes on every tick; slots beyond inst.F are 0.0.
  DECISION fp32  the byte identities, and the whole vectors within 16 x 2^29 x the floors (a second set of shapes, not a rounding-level
                 net: tests/test_gpu_exact_parity_a.py says why).
  PREDICTION     sample 1 of x, xd, xz is the post-tick state by bytes; all samples of all four rows within 16 x floor_pred of
                 horizon_a.predict_exact run on the decision and state THIS call returned (the prediction's error apart from the solve's);
                 an instance with a bad record (ds >= step) is all NaN, its neighbours untouched.
  WORKING SET    read off the prediction (fp64, status 0): the rows the fixture's ws marks active sit on the band edge of the marked sign
                 within 1e-7 (1 + w / 2) (the header's unverified-point threshold), every other row is inside the band.
Every measured maximum and its ratio to the floor goes through _record_maxima."""
import os

import numpy as np
import pytest

from helpers import exact_tick_a as X
from helpers import horizon_a as H
from test_gpu_formulation_a import _record_maxima, q_from_dev, q_to_dev
from test_gpu_exact_parity_a import FORMS, F32_FORMS, KNOBS, PLAIN_GROUPS, LOOP_GROUPS, handle, on_dev

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF4DEAD5EED0A0A          # a NaN no kernel writes (the prediction's own is the quiet NaN 0x7ff8000000000000)
GUARD = 64
HFORMS = ("wave", "block", "cold", "hist")
_floors = {}


def floors(group):
    if not _floors:
        z = np.load(os.path.join(X.GOLDEN, "formA_horizon_floors.npz"))
        _floors.update({k: z[k] for k in z.files})
    return float(_floors[f"{group}_floor_u"]), float(_floors[f"{group}_floor_f"]), np.array(_floors[f"{group}_floor_pred"])


@pytest.fixture(scope="module")
def FA(built_libs):
    import torch
    assert torch.cuda.is_available()
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    return FA


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def guarded(n):
    import torch
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda:0")


def check_guarded(buf, n, what):
    import torch
    torch.cuda.synchronize()
    bits = buf.cpu().numpy()
    assert (bits[n:] == SENTINEL).all(), f"{what}: guard doubles overwritten"
    assert not (bits[:n] == SENTINEL).any(), (f"{what}: slots left as found", np.flatnonzero(bits[:n] == SENTINEL)[:8])
    return bits[:n].view(np.float64)


def horizon_tick(FA, gen, state_dev, push=None, inst=None, want_pred=True):
    """One ismpc_a_tick_batch_horizon_device call into sentinel-filled, guarded buffers: (OUT_A [b], dec [b, 2, C + F], pred [b, 2, 4, C])."""
    import torch
    b = state_dev.shape[0]
    C, F = gen.horizon_shape()
    nd, npr = b * 2 * (C + F), b * 2 * 4 * C
    dec, pred = guarded(nd), guarded(npr) if want_pred else None
    out = torch.empty((b, 80), dtype=torch.uint8, device="cuda:0")
    gen.tick_horizon_device(b, state_dev.data_ptr(), out.data_ptr(), dec.data_ptr(), pred.data_ptr() if want_pred else None,
                            push.data_ptr() if push is not None else None, inst.data_ptr() if inst is not None else None,
                            torch.cuda.current_stream().cuda_stream)
    d = check_guarded(dec, nd, "dec").reshape(b, 2, C + F)
    p = check_guarded(pred, npr, "pred").reshape(b, 2, 4, C) if want_pred else None
    return q_from_dev(out, FA.OUT_A), d, p


def run_group(FA, fx, precision, hist, horizon, inst_edit=None):
    """Every tick of a fixture through its case's handle, as test_gpu_exact_parity_a.run_single_ticks: the plain tick (horizon False) or the
    horizon tick.  Returns dict(out, after, dec, pred, deferred); dec / pred are lists per tick ([2, C + F], [2, 4, C]) of the handle's shape."""
    n = len(fx["case"])
    out, after = np.zeros(n, FA.OUT_A), np.zeros(n, FA.STATE_A)
    dec, pred, deferred = [None] * n, [None] * n, []
    states = fx["state"].view(FA.STATE_A).reshape(-1)
    for case in range(len(fx["params"])):
        sel = np.flatnonzero(fx["case"] == case)
        inst = None
        if fx["has_inst"]:
            gen = handle(FA, fx, case, precision, plans=(0, 1))
            rec = fx["inst"][sel].view(FA.INST_A).reshape(-1).copy()
            if inst_edit is not None:
                inst_edit(rec)
            inst = q_to_dev(rec)
        else:
            gen = handle(FA, fx, case, precision, plans=(int(fx["plan"][sel[0]]),))
        plain = (lambda d, p: gen.tick_inst_torch(d, inst, p)) if inst is not None else gen.tick_torch
        push = on_dev(fx["push"][sel])
        if hist:
            gen.set_warm_history(True)
            plain(q_to_dev(states[sel].copy()), push)
        d = q_to_dev(states[sel].copy())
        if horizon:
            o, dd, pp = horizon_tick(FA, gen, d, push, inst)
            for k, i in enumerate(sel):
                dec[i], pred[i] = dd[k], pp[k]
        else:
            o = q_from_dev(plain(d, push), FA.OUT_A)
        out[sel], after[sel] = o, q_from_dev(d, FA.STATE_A)
        if precision == "f32":
            deferred.append(gen.last_deferred())
        gen.close()
    return dict(out=out, after=after, dec=dec, pred=pred, deferred=deferred)


def tick_par(fx, i):
    insts = fx["inst"].view(X.INST_A).reshape(-1)
    return X.Par(fx["params"][fx["case"][i]], insts[i] if fx["has_inst"] else None)


def check_identities(fx, r):
    """dec[.., 0] / dec[.., C] against out.u0 / out.f0 by bytes on every tick; slots beyond inst.F are 0.0 (bit pattern of +0.0)."""
    for i in range(len(fx["case"])):
        hC, par = int(fx["params"][fx["case"][i]][0]), tick_par(fx, i)
        d = r["dec"][i]
        assert d[:, 0].tobytes() == r["out"]["u0"][i].tobytes(), ("u0", i)
        assert d[:, hC].tobytes() == r["out"]["f0"][i].tobytes(), ("f0", i)
        assert d[:, hC + par.F:].tobytes() == bytes(8 * d[:, hC + par.F:].size), ("slots beyond inst.F", i)


def check_decision(fx, r, group, label, ratio=1.0):
    fu, ff, _ = floors(group)
    eu = ef = 0.0
    for n, i in enumerate(fx["sol_idx"]):
        par = tick_par(fx, i)
        C, F = par.C, par.F
        sol, d = fx["sol"][n], r["dec"][i]
        assert np.isfinite(d).all()
        eu = max(eu, float(np.abs(d[:, :C] - sol[:, :C]).max())); ef = max(ef, float(np.abs(d[:, C:C + F] - sol[:, C:C + F]).max()))
    _record_maxima(f"horizonA:{label}", dict(u=eu, f=ef, ratio_u=eu / (fu * ratio), ratio_f=ef / (ff * ratio)))
    print(f"horizonA[{label}] u={eu:.3e}/{fu * ratio:.3e} f={ef:.3e}/{ff * ratio:.3e}")
    assert eu <= X.BOUND_FACTOR * ratio * fu, (label, "u", eu, fu * ratio)
    assert ef <= X.BOUND_FACTOR * ratio * ff, (label, "f", ef, ff * ratio)


def check_prediction(fx, r, group, label):
    _, _, fp = floors(group)
    states = fx["state"].view(X.STATE_A).reshape(-1)
    e = np.zeros(4)
    for i in range(len(fx["case"])):
        par, p, d = tick_par(fx, i), r["pred"][i], r["dec"][i]
        hC = int(fx["params"][fx["case"][i]][0])
        first = H.first_of(r["after"][i])
        assert p[:, :3, 0].tobytes() == first.tobytes(), ("sample 1 is the post-tick state", i)
        dd = np.concatenate([d[:, :hC], d[:, hC:hC + par.F]], 1)
        want = H.predict_exact(par, states[i], fx["push"][i], dd, first)
        assert np.isfinite(p).all()
        e = np.maximum(e, np.abs(p - want).max(axis=(0, 2)))
    _record_maxima(f"horizonA:{label}:pred", dict(**{k: float(v) for k, v in zip(H.ROWS, e)}, **{f"ratio_{k}": float(v / f) for k, v, f in zip(H.ROWS, e, fp)}))
    print(f"horizonA[{label}] pred " + " ".join(f"{k}={v:.3e}/{f:.3e}" for k, v, f in zip(H.ROWS, e, fp)))
    assert (e <= X.BOUND_FACTOR * fp).all(), (label, e.tolist(), fp.tolist())


def check_working_set(fx, r, label):
    worst_on, least_in = 0.0, np.inf
    for i in range(len(fx["case"])):
        if r["out"]["status"][i] != 0:
            continue
        par, p = tick_par(fx, i), r["pred"][i]
        ws = fx["ws"][i][:, :par.C]
        m, side = H.band_margin(par, p), H.band_side(p)
        act = ws != 0
        assert (np.abs(m[act]) <= 1e-7 * (1 + par.w / 2)).all(), (label, i, "active rows off the band edge", np.abs(m[act]).max())
        assert (side[act] == ws[act]).all(), (label, i, "active rows on the other edge")
        assert (m[~act] > 0).all(), (label, i, "an inactive row outside the band", m[~act].min())
        worst_on = max(worst_on, float(np.abs(m[act]).max()) if act.any() else 0.0)
        least_in = min(least_in, float(m[~act].min()) if (~act).any() else np.inf)          # (a pushed tick can pin every row)
    _record_maxima(f"horizonA:{label}:ws", dict(active_off_edge=worst_on, inactive_slack=least_in))


def same_tick(a, b, label):
    assert a["out"].tobytes() == b["out"].tobytes(), (label, "out differs from the plain tick's")
    assert a["after"].tobytes() == b["after"].tobytes(), (label, "state differs from the plain tick's")
    assert a["deferred"] == b["deferred"], (label, a["deferred"], b["deferred"])


@pytest.mark.parametrize("form", HFORMS)
@pytest.mark.parametrize("group", PLAIN_GROUPS + LOOP_GROUPS)
def test_single_ticks_fp64(FA, group, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    label = f"{group}:{form}"
    r = run_group(FA, fx, "f64", form == "hist", True)
    same_tick(r, run_group(FA, fx, "f64", form == "hist", False), label)
    check_identities(fx, r)
    check_decision(fx, r, group, label)
    check_prediction(fx, r, group, label)
    check_working_set(fx, r, label)


@pytest.mark.parametrize("bucket", [0, 1])
@pytest.mark.parametrize("form", ["wave", "hist"])
def test_per_instance_ticks_fp64(FA, form, bucket, monkeypatch):
    monkeypatch.setenv("ISMPC_A_BUCKET", str(bucket))
    fx = X.load_group("inst_C200")
    label = f"inst_C200:{form}:bucket{bucket}"
    r = run_group(FA, fx, "f64", form == "hist", True)
    same_tick(r, run_group(FA, fx, "f64", form == "hist", False), label)
    check_identities(fx, r)
    check_decision(fx, r, "inst_C200", label)
    check_prediction(fx, r, "inst_C200", label)
    check_working_set(fx, r, label)


@pytest.mark.parametrize("form", list(F32_FORMS))
@pytest.mark.parametrize("group", PLAIN_GROUPS + ("inst_C200",))
def test_single_ticks_fp32(FA, group, form, monkeypatch):
    for k, v in F32_FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    label = f"{group}:f32:{form}"
    r = run_group(FA, fx, "f32", False, True)
    same_tick(r, run_group(FA, fx, "f32", False, False), label)
    check_identities(fx, r)
    check_decision(fx, r, group, label, ratio=X.F32_RATIO)
    check_prediction(fx, r, group, label)


@pytest.mark.parametrize("bucket", [0, 1])
def test_per_instance_ticks_fp32_bucket(FA, bucket, monkeypatch):
    monkeypatch.setenv("ISMPC_A_BUCKET", str(bucket))
    fx = X.load_group("inst_C200")
    label = f"inst_C200:f32:bucket{bucket}"
    r = run_group(FA, fx, "f32", False, True)
    same_tick(r, run_group(FA, fx, "f32", False, False), label)
    check_identities(fx, r)
    check_decision(fx, r, "inst_C200", label, ratio=X.F32_RATIO)


@pytest.mark.parametrize("group", LOOP_GROUPS)
def test_caller_driven_loop_is_the_plain_loop(FA, group):
    """ismpc_a_set_warm_history(h, 1) and one call per tick at batch 1: the loop of horizon ticks against the same loop of plain ticks."""
    fx = X.load_group(group)
    n = len(fx["case"])
    s0 = fx["state"][:1].view(FA.STATE_A).reshape(-1)
    got = []
    for horizon in (True, False):
        gen = handle(FA, fx, 0, plans=(int(fx["plan"][0]),))
        gen.set_warm_history(True)
        st = q_to_dev(s0.copy())
        out, after = np.zeros(n, FA.OUT_A), np.zeros(n, FA.STATE_A)
        C, _ = gen.horizon_shape()
        for t in range(n):
            push = on_dev(fx["push"][t:t + 1])
            if horizon:
                o, d, p = horizon_tick(FA, gen, st, push)
                assert d[0, :, 0].tobytes() == o["u0"][0].tobytes() and d[0, :, C].tobytes() == o["f0"][0].tobytes(), t
                out[t] = o[0]
                after[t] = q_from_dev(st, FA.STATE_A)[0]
                assert p[0, :, :3, 0].tobytes() == H.first_of(after[t]).tobytes(), t
            else:
                out[t] = q_from_dev(gen.tick_torch(st, push), FA.OUT_A)[0]
                after[t] = q_from_dev(st, FA.STATE_A)[0]
        gen.close()
        got.append((out, after))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def test_bad_record_is_nan_and_neighbours_are_untouched(FA):
    """Instances 3 and 10 get ds >= step: ISMPC_A_ST_BAD_INDEX, u = 0, every footstep = out.f0 = the current one, every sample a quiet NaN;
    every other instance's out, state, dec and pred bytes are those of the unedited batch."""
    fx = X.load_group("inst_C200")
    bad = [3, 10]

    def edit(rec):
        rec["ds"][bad] = rec["step"][bad]
    good, r = run_group(FA, fx, "f64", False, True), run_group(FA, fx, "f64", False, True, inst_edit=edit)
    states = fx["state"].view(FA.STATE_A).reshape(-1)
    C = int(fx["params"][0][0])
    for i in range(len(fx["case"])):
        if i in bad:
            assert r["out"]["status"][i] & FA.ST_BAD_INDEX
            assert r["after"][i].tobytes() == states[i].tobytes()
            assert np.isnan(r["pred"][i]).all()
            assert not r["dec"][i][:, :C].any()
            assert np.array_equal(r["dec"][i][:, C:], np.repeat(r["out"]["f0"][i][:, None], r["dec"][i].shape[1] - C, 1))
            assert np.array_equal(r["out"]["f0"][i], [states[i]["cur_x"], states[i]["cur_y"]])
        else:
            for k in ("out", "after", "dec", "pred"):
                assert r[k][i].tobytes() == good[k][i].tobytes(), (k, i)


def test_horizon_shape_and_no_prediction(FA):
    """ismpc_a_horizon_shape on a walk C = 100 F = 3 and a C = 200 F = 6 handle; pred_dev = NULL gives the same tick and decision."""
    g = FA.default_gait(FA.WALK, np.pi / 4, 0.1)
    _, ce = FA.plan(g)
    gen = FA.GaitGenerator(FA.default_params(FA.WALK), ce)
    assert gen.horizon_shape() == (100, 3)
    st = gen.initial_state(g.disp_C, batch=5)
    d1, d2 = q_to_dev(st.copy()), q_to_dev(st.copy())
    o1, dec1, _ = horizon_tick(FA, gen, d1)
    o2, dec2, p2 = horizon_tick(FA, gen, d2, want_pred=False)
    assert p2 is None and o1.tobytes() == o2.tobytes() and dec1.tobytes() == dec2.tobytes() and q_from_dev(d1, FA.STATE_A).tobytes() == q_from_dev(d2, FA.STATE_A).tobytes()
    out, dec, pred = gen.tick_horizon_torch(q_to_dev(st.copy()))
    assert tuple(dec.shape) == (5, 2, 103) and tuple(pred.shape) == (5, 2, 4, 100) and dec.cpu().numpy().tobytes() == dec1.tobytes()
    gen.close()
    gen = FA.GaitGenerator(FA.default_params(FA.TROT, C=200, P=400, F=6), ce)
    assert gen.horizon_shape() == (200, 6)
    gen.close()
