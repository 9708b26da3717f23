"""A user proposal on the host (ptm_set_proposal_callback, a C function) against the same proposal on the device
(ptm_set_proposal_device), us per PT step in one process on one device:
  (a) host proposals, Gaussian target          (b) device proposals, Gaussian target
  (c) device proposals + a device likelihood   (d) the engine's own proposals + the same device likelihood (what (c) stands beside:
                                                   host proposals refuse a device likelihood)
Per shape: 50 warm-up steps each, then BLOCKS timed blocks of 200 steps, the configurations taking turns inside every block round;
a block's time is a host clock around step(200) + sync.  (a) and (b) draw the same numbers: their chains must be equal at the end.
Writes one JSON document (--out).  Usage: python tools/device_proposals_probe.py [--out FILE] [--blocks N]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptmcmc_amd import engine as E  # noqa: E402
from ptmcmc_amd.problems import GaussianProblem  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = [(6, 20, 64), (32, 64, 1024)]     # dimensions x rungs x walkers: the LISA example's shape; a full device
WARM, STEPS = 50, 200


class ScriptedUser(C.Structure):
    _fields_ = [("scale_dev", C.c_void_p), ("accepted_out_dev", C.c_void_p), ("rung_out_dev", C.c_void_p), ("walker_out_dev", C.c_void_p),
                ("count_out_dev", C.c_void_p), ("calls", C.c_uint64), ("result_calls", C.c_uint64), ("last_step", C.c_uint64 * 4)]


def build(d):
    so = os.path.join(d, "libdevprop_probe.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "scripted_device_proposal.hip"), os.path.join(ROOT, "tools", "probes", "device_proposals_probe.hip"),
                           "-o", so])
    return C.CDLL(so)


def fptr(f):
    return C.cast(f, C.c_void_p).value


def run_shape(lib, D, Nt, W, blocks):
    pr = GaussianProblem(D, Nt, 1e3)
    scale = np.ascontiguousarray(2.0 / np.sqrt(D) / np.sqrt(np.maximum(pr.beta, 0.02)) * np.sqrt(np.diag(pr.cov).mean()))
    sdev = E.DeviceBuffer(scale.nbytes)
    sdev.copy_from(scale.ctypes.data)
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))
    keep, engines = [sdev, scale], {}
    for name in ("a_host_proposals", "b_device_proposals", "c_device_proposals_device_likelihood", "d_own_proposals_device_likelihood"):
        eng = E.Engine(D, Nt, W, seed=0x5EED0001, swap_rate=0.1)
        pr.configure(eng, E.PROP_DIAG)
        if name[0] in "cd":
            eng.set_target_device_c(fptr(lib.probe_loglike_device))
        if name[0] == "a":
            eng._keep.append(scale)
            E._chk(eng.L.ptm_set_proposal_callback(eng.h, C.c_void_p(fptr(lib.probe_propose_host)), None, C.c_void_p(scale.ctypes.data)))
        elif name[0] in "bc":
            u = ScriptedUser(sdev.ptr, None, None, None, None, 0, 0)
            keep.append(u)
            eng.set_proposal_device_c(fptr(lib.scripted_propose_device), None, user=C.addressof(u))
        eng.set_states(x0)
        engines[name] = eng
    times = {k: [] for k in engines}
    for k, eng in engines.items():
        eng.step(WARM); eng.sync()
    for _ in range(blocks):
        for k, eng in engines.items():
            t0 = time.perf_counter()
            eng.step(STEPS); eng.sync()
            times[k].append((time.perf_counter() - t0) / STEPS * 1e6)
    a, b = engines["a_host_proposals"], engines["b_device_proposals"]
    same = bool(np.array_equal(a.states(), b.states()) and np.array_equal(a.naccept, b.naccept))
    out = {"shape": {"dim": D, "rungs": Nt, "walkers": W, "chains": Nt * W}, "host_and_device_chains_equal": same, "configs": {}}
    for k, eng in engines.items():
        t = np.array(times[k])
        acc = float((eng.naccept.sum() - eng.Nc) / max(1, eng.ntries.sum() - eng.Nc))
        out["configs"][k] = {"us_per_step_median": round(float(np.median(t)), 2), "us_per_step_min": round(float(t.min()), 2),
                             "us_per_step_max": round(float(t.max()), 2), "blocks_us_per_step": [round(float(v), 2) for v in t],
                             "step_kernel": eng.step_kernel_name, "acceptance": round(acc, 4)}
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="device_proposals.json")
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    if E.device_count() < 1:
        raise SystemExit("needs an MI355X: no gfx950 device visible")
    with tempfile.TemporaryDirectory() as d:
        lib = build(d)
        doc = {"what": "us per PT step, host proposals (C callback) against the same proposal on the device; median / min / max of the timed blocks",
               "method": "%d warm-up steps, then %d blocks of %d steps per configuration, the configurations alternating inside every round of blocks, "
                         "one process; a block is a host clock around step(%d) + sync" % (WARM, a.blocks, STEPS, STEPS),
               "proposal": "scripted proposal of examples/scripted_device_proposal.hip (splitmix64 uniforms, a jump per dimension, scripted ratios, types, validity)",
               "shapes": [run_shape(lib, D, Nt, W, a.blocks) for D, Nt, W in SHAPES]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
