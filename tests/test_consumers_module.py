"""CPU-only: nrsc5_amd.consumers and nrsc5_amd.engine each import on their own, in either order, and engine still offers every consumer name."""
import os
import subprocess
import sys

import pytest

from nrsc5_amd import consumers, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("HdcConsumer", "PsdConsumer", "SisConsumer", "feed_hdc", "feed_hdc_batch", "feed_psd_batch", "feed_sis_batch",
         "sis_utf8", "sis_text", "_sis_device_info", "sis_event_fields")


@pytest.mark.parametrize("module", ["nrsc5_amd.consumers", "nrsc5_amd.engine"])
def test_imports_first_in_a_fresh_interpreter(module):
    r = subprocess.run([sys.executable, "-c", "import %s" % module], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_engine_offers_the_same_objects():
    for name in MOVED:
        assert getattr(engine, name) is getattr(consumers, name), name
