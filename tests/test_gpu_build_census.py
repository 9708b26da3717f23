"""The census of kernel builds on the GPU: every sweep and step kernel the engine can choose (tests/build_census.py names one
configuration per build) reports the table's name, string for string, and then computes chains bit for bit the checker's -- three
rounds of three PT steps, two plain sweeps, two more PT steps, with states, scalars, counters, type codes, the last step's exchange
log, the swap counters, the temperatures of evolving ladders, every saved row and MAP where they are tracked and the adaptive state
where a set adapts compared after each.  The cases that need an environment switch of the engine run in one child process per switch
(tests/census_worker.py), started on first use."""
import json
import os
import subprocess
import sys

import pytest

import build_census as BC
import census_util as CU

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_children = {}


def child_lines(switch):
    """(status, lines by case name, the end of stderr) of the switch's child process.  The child is started ONCE, by the first case that
    asks, whatever becomes of it: one that ran out of time or could not be started is remembered as such, and the other cases fail from
    the record without starting anything."""
    if switch not in _children:
        var, value = switch.split("=")
        env = dict(os.environ)
        env[var] = value
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "census_worker.py"), switch], env=env, capture_output=True, text=True, timeout=300)
            status, out, err = "exit status %d" % r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
            status, out, err = "timed out after 300 s", text(e.stdout), text(e.stderr)
        except Exception as e:
            status, out, err = "not started: %r" % (e,), "", ""
        lines = {}
        for ln in out.splitlines():
            if ln.startswith("{"):
                try:
                    d = json.loads(ln)
                except ValueError:      # (a line cut off by the time limit)
                    continue
                lines[d["name"]] = d
        _children[switch] = (status, lines, err[-2000:])
    return _children[switch]


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_the_build_computes_the_checkers_chains(name):
    c = BC.CASES[name]
    if c.get("env"):
        status, lines, err = child_lines(c["env"])
        assert name in lines, "the child process of %s (%s) printed no line for this case\n%s" % (c["env"], status, err)
        assert lines[name]["ok"], lines[name]["error"]
        seen = lines[name]
    else:
        seen = CU.run_case(name, c)
    assert 0 < seen["accepted"] < seen["tries"]
