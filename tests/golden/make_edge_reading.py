"""Records the numpy second reading (tests/second_reading.py: ref_compute_incc, ref_cost_func) of the seeds of
tests/edge_scenes.py's groups -- every mixed-scale seed at working levels 0 and 1, 600 seeds of each well-conditioned class of the
patchwork scene -- into tests/golden/edge_second_reading.npz: per group incc (n x 2: plain, robust) and cost (n: cost_func of the
oracle's preProcess output at its own encode()); NaN where a seed is left out or preProcess drops it.  Minutes of numpy, one process per group.  Run from the
repository root: python tests/golden/make_edge_reading.py"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def one(group):
    import edge_scenes as t
    r = t.compute_reading(group)
    return t.group_name(group), r["incc"], r["cost"]


if __name__ == "__main__":
    import edge_scenes as t
    with multiprocessing.Pool(len(t.GROUPS)) as pool:
        out = {}
        for name, incc, cost in pool.map(one, t.GROUPS):
            out[name + "/incc"], out[name + "/cost"] = incc, cost
            print(name, incc.shape[0], "seeds,", int(np.isnan(incc[:, 0]).sum()), "left out,", int((~np.isnan(cost)).sum()), "costs")
    np.savez_compressed(t.GOLDEN, **out)
    print(os.path.getsize(t.GOLDEN), "bytes")
