"""The C++ facade with the reference's regression flags --prop_adapt_rate=0.01 --prop_adapt_more (test/exampleLISA/Makefile): the
sampler's adaptive recipe -- differential evolution beside a nested set of six Gaussians, both sets adapting -- drawn and adapted on
the device, its "Proposal report" showing the device's current shares; PTM_HOST_DE=1 keeps the host-proposal path."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from test_cxx_facade import build

pytestmark = pytest.mark.gpu


def _cold_shares(stdout):
    """the cold rung's line of every "Proposal report": (top shares, nested shares)"""
    out = []
    for block in stdout.split("Proposal report:")[1:]:
        line = [l for l in block.splitlines() if "shares=[" in l][0]
        inner = re.search(r":shares=\[([^\]]*)\]", line).group(1)
        head = re.sub(r":shares=\[[^\]]*\]", "", line.split("shares=[", 1)[1]).rstrip().rstrip("]")
        top = [float(v) for v in head.split(",")]
        out.append((top, [float(v) for v in inner.split(",")]))
    return out


@pytest.mark.parametrize("where", ["device", "host"])
def test_lisa_with_the_reference_regression_flags(where):
    import lisa_toy
    with tempfile.TemporaryDirectory() as d:
        exe, base = os.path.join(d, "ex"), os.path.join(d, "lisa")
        build(exe, "example_lisa.cc")
        env = dict(os.environ)
        env.pop("PTM_HOST_DE", None)
        if where == "host":
            env["PTM_HOST_DE"] = "1"
        r = subprocess.run([exe, "--outname=" + base, "--pt=12", "--nsteps=2000", "--nevery=100", "--save_every=2", "--nskip=2", "--seed=0.25",
                            "--prop_adapt_rate=0.01", "--prop_adapt_more"], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "proposals drawn on the " + where in r.stdout, r.stdout[-2000:]
        reports = _cold_shares(r.stdout)
        assert len(reports) >= 4
        for top, inner in reports:
            assert len(top) == 2 and len(inner) == 6 and abs(sum(top) - 1) < 1e-5 and abs(sum(inner) - 1) < 1e-5, (top, inner)   # (printed to 6 digits)
        assert reports[0] != reports[-1]     # the shares moved over the run
        text = open(base + "_t0.dat").read()
        rows = [l for l in text.splitlines() if l and not l.startswith("#")]
        R = np.array([[float(v) for v in l.replace(":", " ").split()] for l in rows])
        X, ll = R[:, 5:11], R[:, 2]
        want = np.array([lisa_toy.loglike(x) for x in X])
        assert np.allclose(ll, want, rtol=1e-8, atol=1e-5)
        types = set(R[:, 4].astype(int).tolist())
        assert (0 in types or 10 in types) and any(t % 10 == 1 for t in types), types
