"""GPU: a trained ResMLP population replayed in one call (csrc/mlp_population.hip, the device fold of csrc/mlp_fold.h, wtk_mlp_trainer_keep_scored;
DESIGN.md section 25).  The yardstick everywhere is the EXISTING per-model path — `rp.mlp(trainer.folded(e))`, host fold, one wtk_mlp handle and one
mlp_kernel launch per model — compared bit for bit; it is never the code under test.  Shapes: the track has 37 cycles (three 16-sample tiles, the last
one partial), cycle 0's anchor reaches before frame 0, two missed detections cost one sample its first box and another a middle one, one box has an
infinite width."""
import os

import numpy as np
import pytest
import torch

from harness import mlp_population_ref as pr
from harness import mlp_ref
from harness import mlp_train_ref as tr
from wtracker_amd import hip
from wtracker_amd.hip import WtkError
from wtracker_amd.replay import Replay
from wtracker_amd.sim import ExperimentConfig, TimingConfig
from wtracker_amd.training import HipMLPTrainer

pytestmark = pytest.mark.gpu

FRAMES7 = [0, -2, -9, -11, -18, -20, -27]  # the shipped predictors' input frames: in_dim 28
N_FRAMES, N_CYCLES = 332, 37               # 60 frames/s, (100, 40, 50) ms: L = 9, I = 6, P = 3, anchors 9 c + 3
NAN_ROWS = (93, 172, 88)                   # 93: the FIRST box of cycle 10 (and the third of cycle 11); 172: the fourth box of cycle 20; 88: tiny-in's cycle 10
INF_ROWS = (226,)                          # the second box of cycle 25
ARCHS = ["no-blocks", "one-slice-edge", "two-slices", "odd-pingpong", "none-in-block", "tiny-in", "wide-global", "wide-lds"]


@pytest.fixture(scope="module")
def rp(hip_lib):
    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    ec = ExperimentConfig(name="pop", num_frames=N_FRAMES, frames_per_sec=60, orig_resolution=(1600, 1400), px_per_mm=90, init_position=(900, 700))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    r = Replay(pr.synthetic_track(N_FRAMES, 3, NAN_ROWS, INF_ROWS), tc, ec)
    assert (r.L, r.I, r.P, r.n_cycles) == (9, 6, 3, N_CYCLES) and r.n_cycles % 16 != 0 and r.n_cycles > 32
    return r


def _frames(name):
    return ([-5], [9]) if name == "tiny-in" else (FRAMES7, [9])


def _net(arch, seed):
    """mlp_ref.random_rmlp at the first of seed, seed + 7919, ... whose outputs lie in the range the harness asks of a network."""
    while True:
        try:
            return mlp_ref.random_rmlp(**arch, seed=seed)
        except AssertionError:
            seed += 7919


def _models(name, E, seed0=700, edit=None):
    xi, yi = _frames(name)
    out = []
    for e in range(E):
        sd, acts = _net(mlp_ref.arch_args(name), seed0 + e)
        sd = {k: np.array(v) for k, v in sd.items()}
        if edit is not None:
            edit(e, sd)
        out.append(dict(sd, activations=list(acts), input_frames=xi, pred_frames=yi))
    return out


def _same(x, y):
    """Bit equality of two float64 / int arrays, NaN matching NaN."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    n = np.isnan(x)
    return bool(np.array_equal(n, np.isnan(y)) and np.array_equal(x[~n].view(np.int64), y[~n].view(np.int64)))


def _host(t):
    return t.a.cpu().numpy(), t.b.cpu().numpy(), t.valid.cpu().numpy()


def _per_model(rp, trainer, models, best=False):
    """The yardstick: the stacked targets of rp.mlp(trainer.folded(e)) for e in models -> a, b [C, len, 2], valid [C, len]."""
    parts = [_host(rp.mlp(trainer.folded(e, best=best), max_speed=0.9)) for e in models]
    return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))


def _assert_targets_equal(got, want, cols=None):
    a, b, v = got
    if cols is not None:
        a, b, v = a[:, cols], b[:, cols], v[:, cols]
    assert _same(v, want[2]), "valid"
    assert _same(b, want[1]), "b"
    assert _same(a, want[0]), "a"


# ---------------------------------------------------------------------------------------------------------------------------------- fold
def test_device_fold_equals_the_host_fold_of_trained_states(rp):
    """Three steps at batch 19 move the running statistics off their initial values; `best` is the state behind the first step."""
    models = _models("one-slice-edge", 3)
    t = HipMLPTrainer(models, max_batch=19)
    _, _, X, y = tr.make_case(mlp_ref.arch_args("one-slice-edge"), 19, 710)
    X, y = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y)).cuda()
    t.step(X, y)
    t.test_epoch(X, y, batch_size=19, track_best=True, reset_best=True)
    t.step(X, y), t.step(X, y)
    assert not np.array_equal(t.state_dict(0)["model.input.mlp_layer.1.running_var"], models[0]["model.input.mlp_layer.1.running_var"])
    blobs = {w: t.folded_blob(w).cpu().numpy() for w in ("current", "best")}
    assert not np.array_equal(blobs["current"], blobs["best"])
    for w, blob in blobs.items():
        assert blob.shape == (3, mlp_ref.blob_floats(t.folded(0).layers))
        for e in range(3):
            want = pr.pack(t.folded(e, best=(w == "best")).layers)
            assert np.array_equal(blob[e].view(np.uint32), want.view(np.uint32)), (w, e)
    with pytest.raises(WtkError, match="kept by score"):
        t.folded_blob("scored")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("name", ARCHS)
def test_population_targets_equal_the_per_model_path(rp, name):
    t = HipMLPTrainer(_models(name, 3), max_batch=19)
    layers = t.folded(0).layers
    assert mlp_ref.param_path(layers) == mlp_ref.ARCHS[name]["path"]
    got = _host(rp.mlp_population(t, max_speed=0.9))
    want = _per_model(rp, t, range(3))
    _assert_targets_equal(got, want)
    a, b, v = got
    assert a.shape == (N_CYCLES, 3, 2) and v.shape == (N_CYCLES, 3)
    assert (v[0] == 0).all() and (a[0] == 0).all()  # cycle 0 reaches before frame 0
    assert (v[10] == 0).all() and v.sum() > 0 and (v[:, 0] == v[:, 1]).all()
    if name != "tiny-in":
        # frame 93 is also a later box of cycles 11 - 13, frame 172 one of cycles 19 - 21, the infinite width at 226 one of cycles 25 - 27
        assert (v[[1, 2, 11, 12, 13, 19, 20, 21, 25, 26, 27]] == 0).all() and (v[[3, 9, 14, 18, 22, 24, 28, 36]] == 1).all()
        assert np.isnan(b[10]).all()  # the corner of a missed first box, as the per-model path reads it
    # the models differ (which column is which model is what the comparison above checks); tiny-in's 62 blocks drive two of its three models into the clip everywhere
    assert len({a[:, e].tobytes() for e in range(3)}) >= (2 if name == "tiny-in" else 3)
    t.close()


@pytest.mark.parametrize("E", [1, 300])
def test_one_model_and_more_models_than_compute_units(rp, E):
    models = _models("no-blocks", E, seed0=1000)
    t = HipMLPTrainer(models, max_batch=2)
    got = _host(rp.mlp_population(t))
    picks = sorted({0, E // 2, E - 1})
    _assert_targets_equal(got, _per_model(rp, t, picks), cols=picks)
    if E > 1:  # model 299 alone equals itself in the population
        alone = HipMLPTrainer(models[E - 1:], max_batch=2)
        _assert_targets_equal(got, _host(rp.mlp_population(alone)), cols=[E - 1])
        alone.close()
    t.close()


def test_clamp_saturates_and_keeps_nan(rp):
    def edit(e, sd):
        if e == 0:
            sd["model.output.bias"] = np.array([1e6, -1e6], np.float32)
        if e == 1:
            sd["model.output.bias"] = np.array([np.nan, 0.25], np.float32)

    t = HipMLPTrainer(_models("no-blocks", 3, edit=edit), max_batch=2)
    a, b, v = got = _host(rp.mlp_population(t, max_speed=0.9))
    _assert_targets_equal(got, _per_model(rp, t, range(3)))
    bound = float(np.float32(0.9 * (90 / 60) * 9))
    ok = v[:, 0] == 1
    assert ok.sum() > 20
    assert (a[ok, 0, 0] == bound).all() and (a[ok, 0, 1] == -bound).all()
    assert np.isnan(a[ok, 1, 0]).all() and np.isfinite(a[ok, 1, 1]).all()
    assert (a[~ok] == 0).all()
    t.close()


def test_a_list_of_folded_models_gives_the_trainers_targets(rp):
    t = HipMLPTrainer(_models("odd-pingpong", 3), max_batch=19)
    want = _host(rp.mlp_population(t))
    got = _host(rp.mlp_population([t.folded(e) for e in range(3)]))
    _assert_targets_equal(got, want)
    with pytest.raises(ValueError, match="same structure"):
        rp.mlp_population([t.folded(0), HipMLPTrainer(_models("no-blocks", 1), max_batch=2).folded(0)])
    with pytest.raises(ValueError, match="input_frames and pred_frames"):
        rp.mlp_population([t.folded(0, input_frames=[], pred_frames=[9])])
    with pytest.raises(ValueError, match="unknown state"):
        rp.mlp_population(t, which="latest")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- end to end
def test_replay_of_a_population_equals_the_replays_of_its_models(hip_lib, golden_dir):
    """The shipped 100 ms predictor's structure on the golden track at cycle length 9 (test_gpu_replay's case): model 0 is the shipped predictor."""
    from test_gpu_replay import make_replay

    rpg, tc, ec = make_replay(golden_dir, (100, 40, 50))
    path = os.path.join(golden_dir, "resmlp_100ms.npz")
    sd, acts = mlp_ref.fixture_network(path)
    z = np.load(path)
    rng = np.random.default_rng(5)
    models = []
    for e in range(3):
        m = {k: np.array(v) for k, v in sd.items()}
        if e:
            for k in m:
                if k.endswith(".0.weight") or k == "model.output.weight":
                    m[k] = (m[k] * rng.uniform(0.8, 1.2, size=m[k].shape)).astype(np.float32)
        models.append(dict(m, activations=acts, input_frames=z["input_frames"].tolist(), pred_frames=z["pred_frames"].tolist()))
    t = HipMLPTrainer(models, max_batch=2)
    pop = rpg.mlp_population(t)
    res = rpg.run(pop, rows=range(3))
    obj = {k: rpg.objective(pop, k).cpu().numpy() for k in ("trimmed_bbox_error", "bbox_error", "mse_error", "non_perfect")}
    for e in range(3):
        one = rpg.run(rpg.mlp(t.folded(e)))
        assert np.array_equal(res.moves[e], one.moves[0]) and np.array_equal(res.positions[e], one.positions[0])
        assert np.array_equal(res.row_array(e), one.row_array(0))
        for f in ("bbox_error_sum", "rows", "trimmed_bbox_error_sum", "trimmed_rows", "non_perfect_rows", "mse_error_sum"):
            assert getattr(res.summary, f)[e] == getattr(one.summary, f)[0], f
        assert obj["trimmed_bbox_error"][e] == one.summary.trimmed_mean_bbox_error[0] and obj["bbox_error"][e] == one.summary.mean_bbox_error[0]
        assert obj["mse_error"][e] == one.summary.mean_mse_error[0] and obj["non_perfect"][e] == one.summary.non_perfect[0]
    assert len({res.moves[e].tobytes() for e in range(3)}) == 3
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- keep_scored
def test_keep_scored_follows_the_rule(rp):
    """Model 0: a decrease, a tie, a NaN, a later lower value.  Model 1: +inf first (nothing stored), then a value, a NaN, a tie, a higher value.
    Model 2: masked by `active` from the second call on.  Model 3: never a finite score — the slot stays the initial state."""
    inf, nan = float("inf"), float("nan")
    scores = [[5.0, inf, 1.0, nan], [3.0, 2.0, 0.5, nan], [3.0, nan, 0.25, -inf], [nan, 2.0, 0.125, inf], [1.0, 4.0, 0.0, -inf]]
    active = [None, [1, 1, 0, 1], [1, 1, 0, 1], [1, 1, 0, 1], [1, 1, 0, 1]]
    sd, acts, X, y = tr.make_case(tr.TINY, 19, 720)
    t = HipMLPTrainer([dict(_net(tr.TINY, 720 + e)[0], activations=list(acts)) for e in range(4)], max_batch=19)
    X, y = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y)).cuda()
    state0, steps0 = t._get(0)
    got, got_steps = t._get(4)
    assert np.array_equal(got, state0) and (got_steps == 0).all()  # before any call: the initial state
    assert (t.scores()[1] == 0).all() and np.isnan(t.scores()[0]).all()
    kept = dict(state=state0.copy(), steps=steps0.copy(), score=np.full(4, nan), has=np.zeros(4, np.int32))
    for s, act in zip(scores, active):
        t.step(X, y)
        state, steps = t._get(0)
        pr.keep_scored_model(state, steps, s, act, kept)
        t.keep_scored(torch.tensor(s, dtype=torch.float64, device="cuda"), None if act is None else torch.tensor(act, dtype=torch.int32, device="cuda"))
        got, got_steps = t._get(4)
        best, has = t.scores()
        assert np.array_equal(got.view(np.uint32), kept["state"].view(np.uint32)) and np.array_equal(got_steps, kept["steps"])
        assert np.array_equal(has, kept["has"]) and _same(best, kept["score"])
    assert kept["steps"].tolist() == [5, 2, 1, 0] and kept["has"].tolist() == [1, 1, 1, 0] and kept["score"][:3].tolist() == [1.0, 2.0, 1.0]
    sd_scored = t.state_dict(1, best="scored")
    assert np.array_equal(sd_scored["model.output.weight"].ravel(), kept["state"][1][t.n_train - 2 * 16 - 2:t.n_train - 2])
    with pytest.raises(ValueError, match="float64"):
        t.keep_scored(torch.zeros(4, device="cuda"))
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- fit
def test_fit_scores_every_epoch_in_the_closed_loop(rp):
    """3 epochs, E = 2, one-slice-edge, batch 19: the scores are those of the slow path on a second trainer stepped epoch by epoch with the same orders;
    the kept state is the arg-min epoch's; the fit itself computes what it computes without `closed_loop`."""
    E, n, n_test, epochs = 2, 57, 38, 3
    arch = mlp_ref.arch_args("one-slice-edge")
    _, _, X, y = tr.make_case(arch, n + n_test, 730)
    X, y = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y) * 0.1).cuda()
    Xtr, ytr, Xte, yte = X[:n].contiguous(), y[:n].contiguous(), X[n:].contiguous(), y[n:].contiguous()

    def order(epoch):
        return torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(100 * epoch + e)) for e in range(E)]).to(torch.int32)

    make = lambda: HipMLPTrainer(_models("one-slice-edge", E, seed0=740), max_batch=19, lr=1e-3)  # noqa: E731
    t1, t2, t3 = make(), make(), make()
    r1 = t1.fit(Xtr, ytr, Xte, yte, epochs, batch_size=19, order=order, closed_loop=rp)
    r3 = t3.fit(Xtr, ytr, Xte, yte, epochs, batch_size=19, order=order)
    slow, snaps = np.zeros((epochs, E)), []
    for ep in range(epochs):
        t2.train_epoch(Xtr, ytr, order(ep), 19)
        t2.test_epoch(Xte, yte, 19, track_best=True, reset_best=ep == 0)
        snaps.append([t2.state_dict(e) for e in range(E)])
        for e in range(E):
            slow[ep, e] = rp.run(rp.mlp(t2.folded(e), max_speed=0.9)).summary.trimmed_mean_bbox_error[0]
    print(f"\n[mlp_population] closed-loop trimmed bbox error per epoch and model:\n{slow}")
    assert np.isfinite(slow).all()
    for e in range(E):
        assert r1[e].closed_loop == [float(v) for v in slow[:, e]] and r3[e].closed_loop == []
        assert r1[e].train_loss == r3[e].train_loss and r1[e].test_loss == r3[e].test_loss
        want = snaps[int(np.argmin(slow[:, e]))][e]
        got = t1.state_dict(e, best="scored")
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
        a, b = t1.state_dict(e), t3.state_dict(e)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        a, b = t1.state_dict(e, best=True), t3.state_dict(e, best=True)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    best, has = t1.scores()
    assert has.tolist() == [1, 1] and best.tolist() == slow.min(axis=0).tolist()
    # ... and the population of kept states replays to those scores
    again = rp.objective(rp.mlp_population(t1, which="scored")).cpu().numpy()
    assert again.tolist() == best.tolist()
    for t in (t1, t2, t3):
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- stop word, refusals
def _raw_call(rp, t, stop=None, **over):
    """wtk_replay_mlp_targets with sentinel-filled outputs; returns (outputs before, outputs after, error or None)."""
    layers, n_blocks, per_block = t.blob_structure()
    C = rp.n_cycles
    kw = dict(layers=layers, n_blocks=n_blocks, per_block=per_block, blob=t.folded_blob("current"), E=t.E, track32=rp.track.to(torch.float32).contiguous(),
              track=rp.track, n_track=rp.n_track, anchors=(rp._cycles * rp.L + (rp.I - rp.P)).contiguous(), C=C, frames=FRAMES7, bound=12.0,
              a=torch.full((C, t.E, 2), -7.0, dtype=torch.float64, device="cuda"), b=torch.full((C, t.E, 2), -7.0, dtype=torch.float64, device="cuda"),
              valid=torch.full((C, t.E), -7, dtype=torch.int32, device="cuda"))
    outs = [kw["a"], kw["b"], kw["valid"]]
    kw.update(over)
    err = None
    try:
        hip.replay_mlp_targets(kw["layers"], kw["n_blocks"], kw["per_block"], kw["blob"], kw["E"], kw["track32"], kw["track"], kw["n_track"], kw["anchors"], kw["C"],
                               kw["frames"], kw["bound"], kw["a"], kw["b"], kw["valid"], stop_dev=stop, stream=torch.cuda.current_stream().cuda_stream)
    except WtkError as e:
        err = str(e)
    torch.cuda.synchronize()
    return outs, err


def _untouched(outs):
    return all(bool((o == -7).all()) for o in outs)


def test_stop_word_and_refusals_leave_the_outputs_alone(rp):
    t = HipMLPTrainer(_models("no-blocks", 2), max_batch=2)
    outs, err = _raw_call(rp, t)
    assert err is None and not _untouched(outs) and bool((outs[2] != -7).all())  # the call itself works: every (cycle, model) is written
    outs, err = _raw_call(rp, t, stop=torch.ones(1, dtype=torch.int32, device="cuda"))
    assert err is None and _untouched(outs)
    outs, err = _raw_call(rp, t, stop=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert err is None and not _untouched(outs)
    L = hip._MlpTrainLayer
    four_out = (L * 2)(L(28, 40, 1, 0), L(40, 4, 0, 0))
    no_return = (L * 4)(L(28, 40, 1, 1), L(40, 24, 1, 1), L(24, 36, 1, 1), L(40, 2, 0, 0))
    cases = [("out_dim", dict(layers=four_out)), ("n_in", dict(frames=FRAMES7[:6])), ("n_in", dict(frames=[0])), ("n_in", dict(frames=list(range(17)))),
             ("models", dict(E=0)), ("models", dict(E=-3)), ("residual dim", dict(layers=no_return, n_blocks=1, per_block=2)),
             ("n_layers", dict(n_blocks=1, per_block=1)), ("null", dict(a=None)), ("null", dict(blob=None)), ("null", dict(valid=None)),
             ("null", dict(track=None)), ("n_cycles", dict(C=0))]
    for match, over in cases:
        outs, err = _raw_call(rp, t, **over)
        assert err is not None and match in err, (match, err)
        assert _untouched(outs), match
    t.close()
