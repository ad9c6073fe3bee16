"""bench.py's command line: what lives behind --full."""
import os
import subprocess
import sys

BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")


def _bench(*argv):
    return subprocess.run([sys.executable, BENCH, *argv], capture_output=True, text=True, timeout=120)


def test_no_train_needs_full():
    """--no-train leaves only legs that live behind --full: without it, a usage error
    before anything touches a device."""
    r = _bench("--no-train")
    assert r.returncode == 2
    assert "--full" in r.stderr
