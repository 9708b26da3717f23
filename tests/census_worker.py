"""Child process of tests/test_gpu_build_census.py: every case of the census of kernel builds (tests/build_census.py) that needs one
environment switch of the engine, which reads its switches once per process.  Prints one JSON line per case: what the case saw, or the
assertion it failed.  usage: SWITCH=VALUE python census_worker.py SWITCH=VALUE [aged]   (aged: the cases late in a run,
census_util.run_case_aged, for tests/test_gpu_late_run.py)"""
import json
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    switch = sys.argv[1]
    var, value = switch.split("=")
    assert os.environ.get(var) == value, "start this worker with %s in its environment" % switch
    import build_census as BC
    import census_util as CU
    run = CU.run_case_aged if sys.argv[2:] == ["aged"] else CU.run_case
    for name, c in BC.CASES.items():
        if c.get("env") != switch:
            continue
        try:
            out = dict(run(name, c), ok=True)
        except AssertionError:
            out = dict(name=name, ok=False, error=traceback.format_exc()[-1500:])
        except Exception:
            # not a comparison that failed but the engine or the device: nothing more is started on it
            print(json.dumps(dict(name=name, ok=False, error=traceback.format_exc()[-1500:])), flush=True)
            sys.exit(1)
        print(json.dumps(out), flush=True)
