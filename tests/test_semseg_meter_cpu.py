"""CPU suite: the host arithmetic of the stage-1 evaluation - `semseg_scores` / `SemsegMeter.add_counts` /
`synchronize_between_processes` (semseg_evaluation.py:40-69) and `TrainerAE.compute_metrics`' name check (trainers_ae.py:561-567).
The device counters are covered by tests/test_semseg_eval_gpu.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import semseg_ref as ref


def _random_case(K, n, seed, ignore_index):
    g = np.random.RandomState(seed)
    gt = g.randint(0, K + 3, n)                    # labels >= K appear
    gt[g.rand(n) < 0.2] = ignore_index             # ignore pixels
    pred = np.where(g.rand(n) < 0.6, gt, g.randint(0, K + 3, n))
    pred[g.rand(n) < 0.1] = ignore_index           # predictions equal to the ignore index
    absent = K // 2                                 # a class absent from both
    gt[gt == absent] = 0
    pred[pred == absent] = 0
    return pred, gt, absent


@pytest.mark.parametrize("K,ignore_index", [(5, 255), (128, 0), (7, 3)])
def test_scores_match_brute_force(K, ignore_index):
    from ldmseg_amd.evaluations import SemsegMeter, semseg_scores
    pred, gt, absent = _random_case(K, 4000, K, ignore_index)
    counts = ref.meter_counts(pred, gt, K, ignore_index)
    # the per-pixel form of the rule (what the kernels implement) against the per-class masked sums
    per_pixel = np.zeros_like(counts)
    for q, t in zip(pred, gt):
        if t == ignore_index:
            continue
        if q == t:
            if 0 <= t < K:
                per_pixel[0, t] += 1
        else:
            if 0 <= t < K:
                per_pixel[2, t] += 1
            if 0 <= q < K:
                per_pixel[1, q] += 1
    assert np.array_equal(per_pixel, counts)
    if absent != ignore_index and absent != 0:
        assert counts[:, absent].sum() == 0
    want = ref.meter_scores(counts)
    got = semseg_scores(*counts)
    assert got["jaccards_all_categs"] == want["jaccards_all_categs"]
    assert abs(got["mIoU"] - want["mIoU"]) <= K * 2.0 ** -52          # summation order of K float64 terms in [0, 1]
    if absent != ignore_index and absent != 0:
        assert got["jaccards_all_categs"][absent] == 0.0          # an absent class drags the mean down, as in the reference
    m = SemsegMeter(K, [str(i) for i in range(K)], has_bg=False, ignore_index=ignore_index)
    m.add_counts(*counts)
    m.add_counts(*counts)                                          # totals accumulate; the ratio is unchanged
    assert m.return_score(verbose=False, suppress_prints=True)["jaccards_all_categs"] == want["jaccards_all_categs"]
    assert str(m) == "IoU ({0:.2f})".format(100 * want["mIoU"])
    m.reset()
    assert m.tp.sum() == 0 and m.return_score(verbose=False, suppress_prints=True)["mIoU"] == 0.0


def test_denominator_floor_and_background_class():
    from ldmseg_amd.evaluations import SemsegMeter, semseg_scores
    s = semseg_scores([0, 3], [0, 1], [0, 0])
    assert s["jaccards_all_categs"] == [0.0, 0.75] and s["mIoU"] == 0.375         # 0 / max(0, 1e-8) = 0
    m = SemsegMeter(4, ["bg", "a", "b", "c", "d"], has_bg=True)
    assert m.num_classes == 5 and m.tp.shape == (5,) and m.ignore_index == 255
    with pytest.raises(ValueError):
        m.add_counts([1] * 4, [0] * 4, [0] * 4)
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))      # no CPU fallback


def test_verbose_print(capsys):
    from ldmseg_amd.evaluations import SemsegMeter
    m = SemsegMeter(2, ["x", "y"], has_bg=False)
    m.add_counts([1, 0], [1, 0], [0, 0])
    m.return_score(verbose=True, name="val set")
    out = capsys.readouterr().out
    assert "Evaluation for semantic segmentation - val set" in out and "mIoU is 25.00" in out and "IoU class x is 50.00" in out


def test_compute_metrics_rejects_unknown_names():
    from ldmseg_amd.trainers import TrainerAE
    tr = TrainerAE(None)
    with pytest.raises(NotImplementedError):
        tr.compute_metrics(["miou", "dice"], dataloader=[])
    with pytest.raises(NotImplementedError):
        tr.compute_metrics("fid", dataloader=[])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_counts(rank, K):
    g = np.random.RandomState(100 + rank)
    return g.randint(0, 1 << 40, (3, K)).astype(np.int64)          # beyond fp32 / int32: the sum must stay exact


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "latent-diffusion-segmentation_amd"))
    from ldmseg_amd.evaluations import SemsegMeter
    K = 6
    m = SemsegMeter(K, [str(i) for i in range(K)], has_bg=False, ignore_index=0, gpu_idx="cpu")
    m.add_counts(*_rank_counts(rank, K))
    m.synchronize_between_processes()
    q.put((rank, np.stack([m.tp, m.fp, m.fn])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_synchronize_between_processes_gloo():
    from ldmseg_amd.evaluations import SemsegMeter
    m = SemsegMeter(3, ["a", "b", "c"], has_bg=False)
    m.add_counts([1, 2, 3], [0, 0, 0], [1, 1, 1])
    m.synchronize_between_processes()                              # torch.distributed not initialised: nothing happens
    assert m.tp.tolist() == [1, 2, 3]
    world = 2
    ctx = mp.get_context("spawn")
    res = None
    for attempt in range(3):        # (a rendezvous port can be taken between _free_port() and the store's bind)
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            got = dict(q.get(timeout=120) for _ in range(world))
        except Exception:
            got = None
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join(10)
        if got is not None and all(p.exitcode == 0 for p in procs):
            res = got
            break
    assert res is not None, "two gloo ranks did not complete in three attempts"
    want = _rank_counts(0, 6) + _rank_counts(1, 6)
    assert np.array_equal(res[0], want) and np.array_equal(res[1], want)
