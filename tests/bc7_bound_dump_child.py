"""Child process of tests/test_bc7_bound_soundness.py (not a test): loads the bound-dump build of the library (CVTTMI_LIB in
the environment names it), encodes the jobs it is given with a dump buffer set, and writes the records, their count and the
output bytes of every job to one npz.
    python tests/bc7_bound_dump_child.py jobs.json out.npz
jobs.json: {"blocks": path of an npy (N, 16, 4) uint8, "rcp": 17 binary32 bit patterns, "capacity": records,
            "jobs": [{"name", "n": leading blocks to encode, "options": 44 bytes, "env": {name: value}}]}
A job's `env` is in place while its context is created (the hand-over settings are read then)."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HAND_OVER_ENV = ("CVTTMI_BC7_HARD_MIN", "CVTTMI_BC7_HARD_CAP", "CVTTMI_BC7_HARD_DIV")


def main(jobs_path, out_path):
    import torch
    from convectionkernels_amd import api
    spec = json.load(open(jobs_path))
    lib = api.load_library()
    if not hasattr(lib, "cvttmi_bc7_bound_dump_set"):
        raise SystemExit("%s is not a bound-dump build" % os.environ.get("CVTTMI_LIB"))
    lib.cvttmi_bc7_bound_dump_set.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.cvttmi_bc7_bound_dump_count.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    blocks = np.load(spec["blocks"])
    rcp = np.array(spec["rcp"], np.uint32).view(np.float32)
    cap = int(spec["capacity"])
    plan = api.BC7EncodingPlan()
    out = {}
    buf = torch.zeros((cap, 12), dtype=torch.int32, device="cuda:0")
    for job in spec["jobs"]:
        for k in HAND_OVER_ENV:
            os.environ.pop(k, None)
        os.environ.update(job.get("env", {}))
        ctx = api.Context(0)
        ctx.set_rcp_table(rcp)
        opt = api.Options.frombytes(bytes(job["options"]))
        src = torch.from_numpy(blocks[:job["n"]]).to("cuda:0")
        buf.zero_()
        torch.cuda.synchronize()
        assert lib.cvttmi_bc7_bound_dump_set(ctypes.c_void_p(buf.data_ptr()), cap) == 0
        packed = ctx.encode_bc7(src, opt, plan)
        torch.cuda.synchronize()
        count = ctypes.c_uint32()
        assert lib.cvttmi_bc7_bound_dump_count(ctypes.byref(count)) == 0
        assert lib.cvttmi_bc7_bound_dump_set(None, 0) == 0
        kept = min(count.value, cap)
        out["records_" + job["name"]] = buf[:kept].cpu().numpy().view(np.uint32)
        out["count_" + job["name"]] = np.array([count.value], np.uint64)
        out["packed_" + job["name"]] = packed.cpu().numpy()
        print("%s: %d blocks, %d records" % (job["name"], job["n"], count.value), flush=True)
        del ctx
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
