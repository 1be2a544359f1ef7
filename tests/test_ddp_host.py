"""Host side of data-parallel training, no GPU: the plan of the self-launcher (per-rank environment, device under a re-mapped visible-device
list, refusals), the per-rank seed rule, the checksum formula that the GPU test compares the kernel with, the table comparison of
``check_replicas``, and the new configuration key."""
import numpy as np
import pytest


@pytest.fixture
def no_visible_lists(monkeypatch):
    for k in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "HSA_ENABLE_IPC_MODE_LEGACY"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_launch_plan_environment_of_each_rank(no_visible_lists):
    from buddy_amd import dist as bd
    plan = bd.launch_plan(4, "nccl", port=12345, device_count=8)
    assert [it["rank"] for it in plan] == [0, 1, 2, 3]
    for r, it in enumerate(plan):
        assert it["env"] == {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "4", "LOCAL_WORLD_SIZE": "4", "MASTER_ADDR": "127.0.0.1",
                             "MASTER_PORT": "12345", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
        assert it["device"] == r == it["physical_device"]
    # the ranks read it back the way a torchrun-style launcher's environment is read
    no_visible_lists.setenv("RANK", "2"); no_visible_lists.setenv("LOCAL_RANK", "2"); no_visible_lists.setenv("WORLD_SIZE", "4")
    assert bd.env_rank_world() == (2, 2, 4)
    # without a device count and without a visible list the launcher does not ask the GPU: the rank finds its device itself
    assert [it["device"] for it in bd.launch_plan(2, "nccl")] == [None, None]
    # a value the user set for the IPC mode is kept
    no_visible_lists.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "1")
    assert bd.launch_plan(1)[0]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


def test_launch_plan_devices_under_a_remapped_visible_list(no_visible_lists):
    from buddy_amd import dist as bd
    no_visible_lists.setenv("HIP_VISIBLE_DEVICES", "5,2,7")
    plan = bd.launch_plan(3, "nccl")
    assert [it["device"] for it in plan] == [0, 1, 2] and [it["physical_device"] for it in plan] == [5, 2, 7]
    # HIP's list indexes into ROCR's
    no_visible_lists.setenv("ROCR_VISIBLE_DEVICES", "4,5,6,7")
    no_visible_lists.setenv("HIP_VISIBLE_DEVICES", "3,0")
    plan = bd.launch_plan(2, "nccl")
    assert [it["physical_device"] for it in plan] == [7, 4]
    # gloo: the ranks wrap around the visible devices
    plan = bd.launch_plan(5, "gloo")
    assert [it["device"] for it in plan] == [0, 1, 0, 1, 0] and [it["physical_device"] for it in plan] == [7, 4, 7, 4, 7]


def test_launch_plan_refusals(no_visible_lists):
    from buddy_amd import dist as bd
    assert bd.MAX_RANKS == 16
    assert len(bd.launch_plan(16, "gloo", device_count=1)) == 16
    for n in (17, 64, 0, -1):
        with pytest.raises(ValueError, match="1 to 16"):
            bd.launch_plan(n, "gloo", device_count=1)
    with pytest.raises(ValueError) as e:
        bd.launch_plan(4, "nccl", device_count=2, prog="train.py")
    assert str(e.value) == "train.py: 4 RCCL ranks need 4 GPUs, this node shows 2 (--backend gloo lets ranks share a GPU for smoke tests)"
    no_visible_lists.setenv("HIP_VISIBLE_DEVICES", "0")
    with pytest.raises(ValueError, match="2 RCCL ranks need 2 GPUs, this node shows 1"):
        bd.launch_plan(2, "nccl")
    assert len(bd.launch_plan(2, "gloo")) == 2
    with pytest.raises(ValueError, match="backend"):
        bd.launch_plan(2, "mpi", device_count=2)


def test_refusal_message_is_the_benchmark_drivers():
    """the sentence after the program's name is the one bench.py prints for the same condition"""
    import os
    from buddy_amd import dist as bd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    tail = bd.too_few_devices_message("X", 3, 1).split(": ", 1)[1]
    assert tail == "3 RCCL ranks need 3 GPUs, this node shows 1 (--backend gloo lets ranks share a GPU for smoke tests)"
    assert "RCCL ranks need {world} GPUs, this node shows {torch.cuda.device_count()} (--backend gloo lets ranks share a GPU for smoke tests)" in src


def test_rank_seeds_are_distinct_and_rank_zero_is_the_single_process_run():
    from buddy_amd import dist as bd
    assert bd.RANK_SEED_STRIDE >= 1 << 16
    for seed in (0, 1, 42):
        assert bd.rank_seed(seed, 0) == seed
        assert bd.rank_seed(seed, 0, 3) == seed + 3                  # a loader worker keeps adding its id
    workers = [0, 1, 2, 63, 64, 1023, bd.RANK_SEED_STRIDE - 1]
    pairs = {(r, w): bd.rank_seed(1, r, w) for r in range(bd.MAX_RANKS) for w in workers}
    assert len(set(pairs.values())) == len(pairs), "a (rank, worker) pair shares its seed with another"
    assert len({bd.rank_seed(1, r) for r in range(bd.MAX_RANKS)}) == bd.MAX_RANKS
    assert max(pairs.values()) < 2 ** 32                             # numpy.random.seed takes 32 bits
    with pytest.raises(ValueError):
        bd.rank_seed(1, 0, bd.RANK_SEED_STRIDE)


def test_checksum_formula_by_hand():
    from tests.test_hip_optim_scaled import checksum_ref
    # bits: 1.0 = 0x3F800000, -0.0 = 0x80000000, 2.0 = 0x40000000; multipliers 1, 3, 5
    x = np.array([1.0, -0.0, 2.0], np.float32)
    assert checksum_ref(x) == 0x3F800000 * 1 + 0x80000000 * 3 + 0x40000000 * 5 == 12876513280
    assert checksum_ref(np.array([1.0, 0.0, 2.0], np.float32)) == 0x3F800000 + 0x40000000 * 5
    assert checksum_ref(x[::-1].copy()) != checksum_ref(x)
    # wrap-around: n elements of the pattern 0x7F7FFFFF (the largest finite float) sum to 0x7F7FFFFF * n^2, above 2^64 for n = 2^20
    n = 1 << 20
    big = np.full(n, np.float32(3.4028234663852886e38))
    assert big.view(np.uint32)[0] == 0x7F7FFFFF and 0x7F7FFFFF * n * n > 2 ** 64
    assert checksum_ref(big) == (0x7F7FFFFF * n * n) % 2 ** 64


def test_replica_disagreements_names_buffers_and_ranks():
    from buddy_amd.training.fused import REPLICA_BUFFERS, replica_disagreements
    assert REPLICA_BUFFERS == ("param", "exp_avg", "exp_avg_sq", "ema")
    same = [[1, -2, 3, 4]] * 3
    assert replica_disagreements(same) == []
    table = [[1, -2, 3, 4], [1, -2 + 1, 3, 4], [1, -2, 3, 5]]
    assert replica_disagreements(table) == [("exp_avg", [1]), ("ema", [2])]
    assert replica_disagreements([[7, 7, 7, 7]]) == []


def test_replica_check_interval_key():
    from buddy_amd.config import compose_train
    args = compose_train()
    assert "replica_check_interval" in args.exp.keys() and args.exp.replica_check_interval in (None, "None")
    assert compose_train(overrides=["exp.replica_check_interval=0"]).exp.replica_check_interval == 0
    assert "gpus" not in args.exp.keys()          # +exp.gpus=N is an addition on the command line: the default run is one process
