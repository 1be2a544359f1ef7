"""GPU: seeded sampling through the harness (tester.noise.generator = philox: utils/rng.py, csrc/rng.hip).  With one Philox stream per utterance
name, drawn on the GPU, an utterance's result does not depend on the file order, the rank layout or -- up to the batched kernels' round-off --
the batch it is sampled in, for a user of the plain config: no injected noise factory anywhere in this file.  Shapes as tests/test_hip_multirank.py
builds them (nf = 32, T = 2, two operator updates per step, lengths 8192 / 6000 / 8192)."""
import pytest
import torch

from buddy_amd.config import compose
from buddy_amd.instantiate import instantiate
from buddy_amd.synth import synth_clean, synth_rir, synth_state_dict
from buddy_amd.utils.rng import PhiloxStreams

pytestmark = pytest.mark.gpu
LENGTHS = [8192, 6000, 8192]
BASE = ["tester.sampling_params.T=2", "network.nf=32", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled",
        "tester.posterior_sampling.blind_hp.op_updates_per_step=2"]
PHILOX = BASE + ["tester.noise.generator=philox"]


@pytest.fixture(scope="module")
def net():
    n = instantiate(compose(overrides=BASE).network)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(2, 32).items()})
    return n.cuda().eval()


@pytest.fixture(scope="module")
def items():
    return [(synth_clean(u, L), synth_rir(u, 1500), f"u{u}.wav") for u, L in enumerate(LENGTHS)]


def _tester(*a, **k):
    from buddy_amd.testing.tester import Tester
    return Tester(*a, **k)


def _run(net, items, overrides, batch_size=1, rank=0, world_size=1):
    args = compose(overrides=overrides)
    t = _tester(args, net, instantiate(args.diff_params), test_set=items, device="cuda", in_training=True, batch_size=batch_size, rank=rank,
                world_size=world_size)
    t.test_dereverberation("blind_dereverberation", blind=True)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def in_order(net, items):
    """the one-at-a-time run in file order, seed 0: the reference of this file, computed once"""
    t = _run(net, items, PHILOX)
    assert isinstance(t.sampler.noise, PhiloxStreams) and t.sampler.noise.names == ["u2.wav"]
    # draw bookkeeping of one utterance: initialize_x + T steps; phases once; update_H(use_noise) in the constructor and in the harness;
    # op_updates_per_step regulariser draws per step
    assert t.sampler.noise.counters[0] == 1 + 2
    assert t.sampler.operator.noise.counters[1:] == [1, 2, 2 * 2]
    res = dict(t.results)
    assert sorted(res) == ["u0", "u1", "u2"] and all(torch.isfinite(v).all() and v.shape == (L,) for v, L in zip((res["u0"], res["u1"], res["u2"]), LENGTHS))
    return res


def test_file_order_does_not_change_a_result(net, items, in_order):
    rev = dict(_run(net, items[::-1], PHILOX).results)
    for n in in_order:
        assert torch.equal(rev[n], in_order[n]), (n, float((rev[n] - in_order[n]).abs().max()))


def test_two_ranks_equal_the_single_process_run(net, items, in_order, monkeypatch):
    """utterance u -> rank u mod 2: what each rank computes (``results``) is what the single process computes, bit for bit.  No process group: the
    end-of-run gather is replaced by one that only places the rank's own rows."""
    from buddy_amd import dist as bdist

    def local_only(rows, n_items, rank, world, device=None):
        out = [torch.zeros(0) for _ in range(n_items)]
        for r, i in zip(rows, range(rank, n_items, world)):
            out[i] = r
        return out

    monkeypatch.setattr(bdist, "gather_ragged", local_only)
    got = {}
    for rank in (0, 1):
        t = _run(net, items, PHILOX, rank=rank, world_size=2)
        assert [n for n, _ in t.results] == [f"u{u}" for u in range(rank, 3, 2)]
        got.update(dict(t.results))
    assert sorted(got) == sorted(in_order)
    for n in in_order:
        assert torch.equal(got[n], in_order[n]), (n, float((got[n] - in_order[n]).abs().max()))


def test_batch_of_three_against_single_runs(net, items, in_order):
    """batch_size = 3 groups the two 8192-sample utterances into one batch of two and leaves the 6000-sample one alone: same noise per name, so what
    differs is the batched kernels' round-off -- the batched-vs-single bound of tests/test_hip_cli.py (relative 1e-3 of the peak)"""
    got = dict(_run(net, items, PHILOX, batch_size=3).results)
    for n in in_order:
        a, b = got[n].double(), in_order[n].double()
        err = float((a - b).abs().max() / b.abs().max())
        print(f"batch of three vs single, {n}: {err:.2e}")
        assert torch.isfinite(a).all() and err < 1e-3, (n, err)


def test_another_seed_changes_every_output(net, items, in_order):
    got = dict(_run(net, items, PHILOX + ["tester.noise.seed=1"]).results)
    for n in in_order:
        assert torch.isfinite(got[n]).all() and not torch.equal(got[n], in_order[n]), n
        assert float((got[n] - in_order[n]).abs().max()) > 1e-3 * float(in_order[n].abs().max()), n


def test_default_generator_still_runs_to_the_end(net, items):
    t = _run(net, items, BASE + ["tester.noise.generator=torch"])
    assert getattr(t, "noise_factory", None) is None and t.sampler.noise is None
    assert [n for n, _ in t.results] == ["u0", "u1", "u2"] and all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for _, v in t.results)


def test_pooled_observations_sub_batches_one_against_two(net, items):
    """Tester.sample_observed on a pool of four rows (the chunk pool of real recordings): one batch on one stream against two concurrent
    sub-batches, whose noise objects are slices of the pool's.  Same bound as batched against single."""
    clean = [(synth_clean(10 + u, 8192), synth_rir(u, 1500), f"rec_c{u}.wav") for u in range(4)]
    names = [it[2] for it in clean]
    out = []
    for sub in (1, 2):
        args = compose(overrides=PHILOX + [f"+tester.sub_batches={sub}"])
        t = _tester(args, net, instantiate(args.diff_params), test_set=None, device="cuda", in_training=True, batch_size=4)
        _, y, _, _ = t.prepare_batch(clean, blind=False)
        pred, est = t.sample_observed(y, names)
        torch.cuda.synchronize()
        assert (t._concurrent is not None) == (sub > 1) and pred.shape == (4, 8192) and est.shape[0] == 4
        out.append(pred.detach().cpu())
    for b in range(4):
        a, r = out[1][b].double(), out[0][b].double()
        err = float((a - r).abs().max() / r.abs().max())
        print(f"pooled rows, sub_batches 2 vs 1, {names[b]}: {err:.2e}")
        assert torch.isfinite(a).all() and err < 1e-3, (b, err)


def test_long_form_chunks_draw_from_named_streams(net):
    """Tester.dereverberate_long under the installed factory: chunk k of the clip is the stream ``long_c<k>.wav``, and the run repeats bit for bit"""
    L = 20000
    clean, rir = synth_clean(5, L), synth_rir(5, 1500)
    out = []
    for _ in range(2):
        args = compose(overrides=PHILOX)
        t = _tester(args, net, instantiate(args.diff_params), test_set=None, device="cuda", in_training=True)
        _, _, pred = t.dereverberate_long(clean, rir, blind=True, chunk_seconds=0.512, overlap_seconds=0.064)
        torch.cuda.synchronize()
        assert t.sampler.noise.names == ["long_c0.wav", "long_c1.wav", "long_c2.wav"] and t.sampler.noise.counters == [3, 1, 2, 4]
        assert pred.shape == (L,) and torch.isfinite(pred).all()
        out.append(pred.detach().cpu())
    assert torch.equal(out[0], out[1])
