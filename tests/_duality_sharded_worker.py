"""One rank of a row-sharded workspace asked for the duality calls (launched by test_duality_gpu.py; not a test module).

usage: _duality_sharded_worker.py RANK WORLD PORT OUT_JSON
The smallest two-rank setup of test_sharded_gpu.py (generated kind 1, n = 900, host-staged transport); nothing is solved: both
calls refuse a row block before they look at anything else.  Writes the return codes and messages of this rank.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import numpy as np
    import torch
    import torch.distributed as dist
    import osqp_jl_amd as oq
    from osqp_jl_amd import sharded

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    lib = oq.load_library()
    comm = sharded.HostComm(lib=lib)
    m = oq.Model(lib)
    oq.setup_generated(m, 1, 900, 0, 7, comm=comm, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, verbose=False, linsys_solver="pcg")
    rec = {}
    rec["check"] = int(lib.osqp_amd_duality_gap_check(m.workspace, 1))
    rec["check_msg"] = lib.osqp_amd_last_error().decode()
    buf = np.zeros(6)
    rec["duality"] = int(lib.osqp_amd_duality(m.workspace, buf.ctypes.data_as(C.POINTER(C.c_double)), 6))
    rec["duality_msg"] = lib.osqp_amd_last_error().decode()
    with open("%s.%d" % (out, rank), "w") as f:
        json.dump(rec, f)
    oq.clean(m)
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
