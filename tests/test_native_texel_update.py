"""tests/native/TexelUpdateTest.cpp through the native test binary: with HIPR_DEVICE_TEXEL_UPDATE=1 a tick that only rewrites the pixels of the lace image keeps the
scene on the device (scene_update_counts().texel_updates moves, the uploads stay) and the frame that follows is, bit for bit, the frame of a renderer created after
the edit; without the variable the tick takes the full path and the frame is the same."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu


def test_a_pixel_edit_through_the_renderer_class():
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "TexelUpdateFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "[       OK ] TexelUpdateFixture.a_hole_punched_into_the_lace_image_stays_on_the_device" in p.stdout, p.stdout[-4000:]
