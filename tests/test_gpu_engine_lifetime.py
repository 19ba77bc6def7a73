"""mvs_engine_destroy gives back all the device memory an engine took: ten rounds of create, set_views, upload, propagate and destroy
leave the device's free memory within a few MB of where it started."""
import pytest

from mvskit_amd import engine, synth

pytestmark = pytest.mark.gpu


def test_destroy_frees_device_memory(small_multi_scene):
    import torch

    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4)

    def cycle():
        e = engine.Engine(sc.nviews, level=0, minImageNum=2, seed=3)
        e.set_scene(sc)
        e.upload_patches(seeds)
        c = e.propagate(0)
        assert c["patches"] > 0
        e.close()

    cycle()  # the first round loads the code objects and sets up the runtime
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    print(f"device free memory: {free0 / 2**20:.1f} MiB before, {free1 / 2**20:.1f} MiB after 10 engines")
    assert free0 - free1 < 8 << 20, (free0, free1)
