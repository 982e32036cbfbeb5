"""Checkpoint and bit-exact resume of the fused trainer: six steps straight against three steps, save, a FRESH trainer initialised
from another seed, load, three more steps - every state tensor, every derived bf16 image, the scalars and the digests bit for bit,
in every step form and with everything that is keyed by the step count switched on.  Shapes as tests/test_gpu_dp_ranks.py sizes
its problem: 3 slots x 64, a 3 + 3 layer stack, 512 rows, batch 128."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
S, E, N, B, STEPS = 3, 64, 512, 128, 3


@functools.lru_cache(maxsize=None)
def _problem():
    from oracle import dae_oracle as O
    io = S * E
    rng = np.random.default_rng(33)
    data = rng.random((N, io), dtype=np.float32)
    sched = O.layer_schedule(io, io, 3, 3, False, "embedding")
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    # every row lacks at most one slot; run 0 blanks a slot the row has
    present = np.ones((N, S), dtype=np.uint8)
    lacking = rng.permutation(N)[:N // 3]
    present[lacking, rng.integers(0, S, lacking.size)] = 0
    mtu = np.array([rng.choice(np.flatnonzero(present[r])) for r in range(N)], dtype=np.int32).reshape(N, 1)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(2 * STEPS)]
    return {"sched": sched, "data": data, "bm": bm, "mtu": mtu, "order": order, "present": present}


def _legs():
    from codae.tool import HiddenDropout, InputNoise, LRSchedule, Optimizer, SlotContrast, SlotPresence, WeightAverage
    p = _problem()
    return {
        "bf16-chain": dict(precision="bf16", chain=True),
        "bf16-layers": dict(precision="bf16"),
        "f32": dict(precision="f32"),
        "graph": dict(precision="bf16", use_graph=True),
        "keyed-by-step": dict(precision="bf16", n_slots=S, input_noise=InputNoise("gaussian", sigma=0.1, seed=5),
                              hidden_dropout=HiddenDropout(0.25, seed=3), contrast=SlotContrast(negatives=16, seed=9),
                              optimizer=Optimizer("adam", amsgrad=True, schedule=LRSchedule("cosine", warmup=2, total=8, min_factor=0.1)),
                              weight_average=WeightAverage("ema", decay=0.9), tied_weights=True),
        "swap-presence": dict(precision="bf16", n_slots=S, input_noise=InputNoise("swap", p=0.3, seed=7),
                              presence=SlotPresence(p["present"])),
    }


def _trainer(monkeypatch, leg, seed, **more):
    from codae.train import HipEmbeddingTrainer
    p = _problem()
    kw = dict(_legs()[leg] if isinstance(leg, str) else leg)
    kw.update(more)
    if kw.pop("chain", False):
        monkeypatch.delenv("CODAE_NO_CHAIN", raising=False)
    else:
        monkeypatch.setenv("CODAE_NO_CHAIN", "1")
    tr = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3, 1e-4, 1.0,
                             max_batch=B, device=DEV, **kw)
    tr.init_params(seed=seed)
    return tr


def _steps(tr, lo, hi, after=None):
    for idx in _problem()["order"][lo:hi]:
        tr.train_batch(torch.tensor(idx, device=DEV), run=0)
        if after is not None:
            after(tr)


def _bits(t):
    return None if t is None else t.detach().contiguous().view(torch.uint8).cpu().numpy().copy()


def _everything(tr):
    """Every piece the resumed run must share with the straight one, as raw bytes / plain numbers."""
    eng = tr.engine
    out = {n: _bits(t) for n, t in eng.state_tensors().items()}
    out["shadow"], out["shadow_t"] = _bits(eng.shadow), _bits(eng.shadow_t)
    if eng.weight_avg is not None:
        eng.sync_average()
        out["avg_shadow"] = _bits(eng.avg_shadow)
        out["weight_avg_synced"] = _bits(eng.weight_avg)
    out["loss_gnorm"] = np.asarray(tr.last_loss_and_grad_norm())
    out["epoch_sums"] = np.asarray(tr.epoch_sums(reset=False))
    d = tr.state_digest()
    out["digest_all"] = np.asarray(d["all"], dtype=np.uint64)
    out["step_count"] = np.asarray([eng.step_count])
    return out


def _assert_same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8) if a[k].dtype != np.uint8 else a[k],
                                                               b[k].view(np.uint8) if b[k].dtype != np.uint8 else b[k]), k


@pytest.mark.parametrize("leg", ["bf16-chain", "bf16-layers", "f32", "graph", "keyed-by-step", "swap-presence"])
def test_resumed_run_has_the_bits_of_the_uninterrupted_run(tmp_path, monkeypatch, leg):
    straight = _trainer(monkeypatch, leg, seed=1)
    if leg == "bf16-chain":
        assert straight.engine.step_path(B) == "chain"
    _steps(straight, 0, 2 * STEPS)
    want = _everything(straight)

    first = _trainer(monkeypatch, leg, seed=1)
    _steps(first, 0, STEPS)
    path = str(tmp_path / "c.npz")
    assert first.save(path, extra={"who": leg}) == os.path.getsize(path)
    at_save = first.state_digest()
    del first

    resumed = _trainer(monkeypatch, leg, seed=2)                      # other initial weights: nothing may survive the load
    assert resumed.state_digest()["params"] != at_save["params"]
    meta = resumed.load(path)
    assert meta["extra"] == {"who": leg} and meta["step_count"] == STEPS == resumed.engine.step_count
    assert resumed.state_digest() == at_save
    _steps(resumed, STEPS, 2 * STEPS)
    _assert_same(want, _everything(resumed))
    if leg == "graph":
        assert resumed.engine.graph_captures() == 1 and straight.engine.graph_captures() == 1
    if leg == "keyed-by-step":
        assert set(meta["optional"]) == {"adam_vmax", "weight_avg"} and meta["tied_weights"] and meta["amsgrad"]
        assert resumed.current_lr() == straight.current_lr() != 1e-3


def test_loaded_shadows_have_the_bits_the_update_kernels_left(tmp_path, monkeypatch):
    """The bf16 images are derived, not stored: right after load() - before any further step - they are the writer's."""
    for leg in ("bf16-chain", "keyed-by-step"):
        a = _trainer(monkeypatch, leg, seed=1)
        _steps(a, 0, STEPS)
        path = str(tmp_path / (leg + ".npz"))
        a.save(path)
        b = _trainer(monkeypatch, leg, seed=2)
        b.load(path)
        for name in ("shadow", "shadow_t"):
            assert np.array_equal(_bits(getattr(a.engine, name)), _bits(getattr(b.engine, name))), (leg, name)
        if a.engine.weight_avg is not None:
            a.engine.sync_average()
            b.engine.sync_average()
            assert np.array_equal(_bits(a.engine.avg_shadow), _bits(b.engine.avg_shadow))
            assert np.array_equal(_bits(a.engine.weight_avg), _bits(b.engine.weight_avg))


def test_snapshots_after_every_step_change_nothing(monkeypatch):
    plain = _trainer(monkeypatch, "keyed-by-step", seed=1)
    _steps(plain, 0, 2 * STEPS)
    watched = _trainer(monkeypatch, "keyed-by-step", seed=1)
    _steps(watched, 0, 2 * STEPS, after=lambda tr: tr.snapshot().release())
    _assert_same(_everything(plain), _everything(watched))


def test_snapshot_holds_the_state_at_the_snapshot_not_after_the_later_step(tmp_path, monkeypatch):
    from codae.tool.checkpoint import StateDigest, read_checkpoint
    tr = _trainer(monkeypatch, "bf16-layers", seed=1)
    _steps(tr, 0, 2)
    before = {n: _bits(t) for n, t in tr.engine.state_tensors().items()}
    digest_before = tr.state_digest()
    snap = tr.snapshot()
    _steps(tr, 2, 3)                                                  # enqueued behind the snapshot's kernels
    after = {n: _bits(t) for n, t in tr.engine.state_tensors().items()}
    assert not np.array_equal(before["params"], after["params"])
    path = str(tmp_path / "s.npz")
    snap.write(path)
    tensors, meta = read_checkpoint(path)                             # (verifies every tensor against meta on the host)
    assert meta["step_count"] == 2 and list(tensors) == list(before)
    for n in before:
        assert np.array_equal(tensors[n].view(np.uint8), before[n]), n
        assert StateDigest.from_hex(meta["digests"][n]) == digest_before[n]
    assert StateDigest.from_hex(meta["all"]) == digest_before["all"]
    tr.snapshot().release()                                           # the staging set is free again


def _rewrite(path, out, change_tensors=None, change_meta=None, drop=()):
    """A copy of a checkpoint with tensors / meta altered on the host, the digests as recorded."""
    from codae.tool.checkpoint import read_checkpoint, write_checkpoint
    tensors, meta = read_checkpoint(path)
    tensors = {n: t.copy() for n, t in tensors.items() if n not in drop}
    if change_tensors:
        change_tensors(tensors)
    if change_meta:
        change_meta(meta)
    write_checkpoint(out, tensors, meta)
    return out


def test_refusals_leave_the_trainer_as_it_was(tmp_path, monkeypatch):
    from codae.hip import HipError
    from codae.tool import Optimizer
    writer = _trainer(monkeypatch, "keyed-by-step", seed=1)
    _steps(writer, 0, 2)
    good = str(tmp_path / "good.npz")
    writer.save(good)

    tr = _trainer(monkeypatch, "keyed-by-step", seed=2)
    _steps(tr, 0, 1)
    mine = tr.state_digest()

    def refused(path, match, who=tr, was=mine, **kw):
        with pytest.raises(HipError, match=match):
            who.load(path, **kw)
        assert who.state_digest() == was and who.engine.step_count == 1

    def other_schedule(meta):
        meta["schedule"][0][1] += 8
    refused(_rewrite(good, str(tmp_path / "sched.npz"), change_meta=other_schedule), "schedule")
    refused(_rewrite(good, str(tmp_path / "novmax.npz"), drop=("adam_vmax",)), "adam_vmax")
    refused(_rewrite(good, str(tmp_path / "noavg.npz"), drop=("weight_avg",)), "weight_avg")

    def one_ulp(tensors):
        v = tensors["adam_v"].view(np.uint32)
        v[1234] ^= 1
    refused(_rewrite(good, str(tmp_path / "ulp.npz"), change_tensors=one_ulp), "adam_v")
    refused(_rewrite(good, str(tmp_path / "short.npz"), change_tensors=lambda t: t.update(params=t["params"][:-4])), "params")

    # tied in the file, untied in the trainer - and the reverse
    untied_kw = dict(_legs()["keyed-by-step"], tied_weights=False)
    untied = _trainer(monkeypatch, untied_kw, seed=2)
    _steps(untied, 0, 1)
    refused(good, "tied", who=untied, was=untied.state_digest())
    untied_file = str(tmp_path / "untied.npz")
    untied.save(untied_file)
    refused(untied_file, "tied")

    # one staging set: a second snapshot while the first is neither written nor released
    snap = tr.snapshot()
    with pytest.raises(HipError, match="snapshot"):
        tr.snapshot()
    assert tr.state_digest() == mine
    snap.release()
    with pytest.raises(HipError, match="written or released"):
        snap.write(str(tmp_path / "late.npz"))
    tr.snapshot().release()

    # strict=False starts a missing average from the loaded parameters; the good file still loads afterwards
    tr.load(str(tmp_path / "noavg.npz"), strict=False)
    assert tr.state_digest()["weight_avg"] == tr.state_digest()["params"] == writer.state_digest()["params"]
    tr.load(good)
    assert tr.state_digest() == writer.state_digest()
    # without AMSGrad the same file is refused under strict for carrying adam_vmax, and accepted without
    plain_kw = dict(_legs()["keyed-by-step"], optimizer=Optimizer("adam"))
    plain = _trainer(monkeypatch, plain_kw, seed=2)
    with pytest.raises(HipError, match="adam_vmax"):
        plain.load(good)
    plain.load(good, strict=False)
    assert plain.state_digest()["adam_v"] == writer.state_digest()["adam_v"]


def test_load_for_inference_answers_as_the_training_process(tmp_path, monkeypatch):
    from codae.tool.checkpoint import read_checkpoint, write_checkpoint
    from codae.train import HipEmbeddingTrainer
    p = _problem()
    tr = _trainer(monkeypatch, "keyed-by-step", seed=1)
    _steps(tr, 0, STEPS)
    path = str(tmp_path / "c.npz")
    tr.save(path)
    # the moments are not needed: strip them from the file
    tensors, meta = read_checkpoint(path)
    lean = str(tmp_path / "lean.npz")
    write_checkpoint(lean, {n: t for n, t in tensors.items() if n in ("params", "weight_avg")}, meta)
    rows = torch.arange(40, dtype=torch.int32)
    items = torch.tensor(np.random.default_rng(4).integers(0, N, (24, S)).astype(np.int32))
    for file in (path, lean):
        inf = HipEmbeddingTrainer.load_for_inference(file, torch.tensor(p["data"]), n_slots=S, max_batch=B, device=DEV)
        assert inf.engine.tied_weights and inf.engine.step_count == STEPS
        for weights in ("live", "average"):
            for got, want in zip(inf.complete(rows, 1, 5, weights=weights), tr.complete(rows, 1, 5, weights=weights)):
                assert torch.equal(got, want)
            a, b = inf.score_outfits(items, weights=weights), tr.score_outfits(items, weights=weights)
            assert list(a) == list(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _dp_worker(rank, world, port, out_dir):
    for q in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "mui-deepautoencoder_amd"), HERE):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"], os.environ["CODAE_NO_CHAIN"] = "127.0.0.1", str(port), "1"
    import torch.distributed as dist
    from codae.hip import HipError
    from codae.train import HipEmbeddingTrainer, shard_batch
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = _problem()
        tr = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3, 1e-4,
                                 1.0, max_batch=B, precision="bf16", device=DEV, distributed=True, n_buckets=4)
        tr.init_params(seed=1)
        for idx in p["order"][:STEPS]:
            tr.train_batch(shard_batch(torch.tensor(idx), rank, world).to(DEV).contiguous(), run=0, global_rows=len(idx))
        res = {"after_steps": tr.dp.replicas_agree()}
        if rank == 1:
            b = tr.engine.bias(2)
            b[3:4] = torch.nextafter(b[3:4], torch.full_like(b[3:4], float("inf")))          # one ulp, through a torch op
        res["after_ulp"] = tr.dp.replicas_agree()
        path = os.path.join(out_dir, "dp.npz")
        sums = tr.epoch_sums(reset=False)                 # over both ranks' partial sums
        wrote = tr.save(path)
        res["wrote"] = wrote is not None
        dist.barrier()
        tr.load(path)
        res["after_load"] = tr.dp.replicas_agree()
        res["step_count"] = tr.engine.step_count
        res["sums_kept"] = sums[0] > 0 and tr.epoch_sums(reset=False) == sums          # the file's sums, carried by rank 0 alone
        try:
            sharded = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]),
                                          1e-3, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, distributed=True, n_buckets=4,
                                          sharded_update=True)
            refused = 0
            for call in (lambda: sharded.save(path + ".x"), lambda: sharded.load(path), sharded.dp.replicas_agree):
                try:
                    call()
                except HipError:
                    refused += 1
            res["sharded_refused"] = refused
        except ValueError:
            res["sharded_refused"] = -1
        np.save(os.path.join(out_dir, "res_%d.npy" % rank), np.asarray([int(res[k]) for k in
                                                                        ("after_steps", "after_ulp", "wrote", "after_load", "step_count",
                                                                         "sharded_refused", "sums_kept")]))
    finally:
        dist.destroy_process_group()


def test_replicas_agree_sees_one_ulp_on_one_rank_and_a_load_heals_it(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(tmp_path / ("res_%d.npy" % r)).tolist() for r in range(2))
    #          after_steps, after_ulp, wrote, after_load, step_count, sharded_refused, sums_kept
    assert r0 == [1, 0, 1, 1, STEPS, 3, 1]
    assert r1 == [1, 0, 0, 1, STEPS, 3, 1]
    assert os.listdir(tmp_path / ".") and os.path.exists(tmp_path / "dp.npz") and not os.path.exists(tmp_path / "dp.npz.x")
