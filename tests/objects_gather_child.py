"""Child process of test_objects_are_refused_after_a_gather (never imported by pytest: no test_ prefix).

One rank, a real RCCL communicator created through the C ABI: after Stixels::ComputeBatchGather the object's
d_stixels holds this rank's packed shard, so Stixels::InstanceObjectsBatch refuses, as WorldBatch does; after the next
ComputeBatch it works again.  Prints OBJECTS_GATHER_OK on success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

import helpers  # noqa: E402
from instance_stixels_amd import core, host  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    comm = core.comm_init_rank(1, core.comm_unique_id(), 0)
    n = 2
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=5, n_images=n)
    cfg = case["cfg"]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    big = torch.from_numpy(case["disparity"]).to(dev)
    seg = torch.from_numpy(case["segmentation"]).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road)
    first = st.InstanceObjectsBatch(n)
    st.ComputeBatchGather(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, comm, 0, [n], road_all=road)
    try:
        st.InstanceObjectsBatch(n)
    except ValueError as e:
        assert "there are none" in str(e), e
    else:
        raise AssertionError("InstanceObjectsBatch after ComputeBatchGather must be refused")
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road)
    second = st.InstanceObjectsBatch(n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    st.Finish()
    core.comm_destroy(comm)
    print("OBJECTS_GATHER_OK")


if __name__ == "__main__":
    main()
