"""hfv_verify_frames_host without a GPU: the entry point is declared, exported by the product and the
test library and wrapped in Python; the ABI version stays 3; the chunk-size hook exists in the test
build only; a NULL ctx is -EINVAL before any device work; the run-again rule restated in Python
(tests/frames_hostmem.py) agrees with hfv_frame_locate on every frame of the corpus at every window;
and the corpus puts frames into every class of the rule at every window."""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import pytest

import frames_hostmem as H
import orc
import scion_hfv as hfv

NAME = "hfv_verify_frames_host"
HOOK = "hfv_debug_frames_host_chunk"


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_entry_point_declared_and_exported():
    src = open(os.path.join(orc.ROOT, "include", "scion_hfv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % NAME, src, flags=re.M)
    assert m, NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["hfv_ctx *ctx", "const uint8_t *frames", "size_t slot", "const uint16_t *len",
                    "const uint32_t *ingress_ifindex", "size_t n", "size_t window", "uint8_t *status",
                    "uint64_t *pass_bits", "size_t *retried"]
    assert re.search(r"#define\s+HFV_ABI_VERSION\s+3\b", src)
    for path in (hfv.LIB_PATH, hfv.TEST_LIB_PATH):
        assert NAME in _exports(path), path
    assert hfv.lib().hfv_abi_version() == 3


def test_hook_only_in_the_test_build():
    product = {s for s in _exports(hfv.LIB_PATH) if s.startswith("hfv_debug_")}
    assert HOOK not in product
    assert HOOK in _exports(hfv.TEST_LIB_PATH)
    src = open(os.path.join(orc.ROOT, "include", "scion_hfv.h")).read()
    assert HOOK not in src


def test_python_wrapper():
    sig = inspect.signature(hfv.Ctx.verify_frames_host)
    assert list(sig.parameters) == ["self", "frames", "slot", "lens", "n", "pass_bits", "ingress_ifindex", "status",
                                    "window"]
    assert sig.parameters["ingress_ifindex"].default is None and sig.parameters["status"].default is None
    assert sig.parameters["window"].default == 0


def test_null_ctx_is_einval_without_gpu():
    L = hfv.lib()
    E = -errno.EINVAL
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    r = ctypes.c_size_t(77)
    assert L.hfv_verify_frames_host(None, p, 64, p, None, 1, 0, None, p, ctypes.byref(r)) == E
    assert "NULL" in L.hfv_last_error().decode()
    assert L.hfv_verify_frames_host(None, None, 64, None, None, 0, 0, None, None, None) == E   # even with n == 0
    assert r.value == 77 and not any(buf)                     # nothing written on the failed call


@pytest.mark.parametrize("window", H.WINDOWS)
def test_model_against_frame_locate(window):
    """Final: the clamped call is the whole call.  Run again: the clamped call stops (status 17 or 26,
    no field found past the model's) where the model says the next header passes the bytes present."""
    frames, lens, _, names = H.corpus()
    slot = frames.shape[1]
    for i in range(len(frames)):
        row, end = bytes(frames[i]), min(int(lens[i]), slot)
        kind, clamped, whole = H.classify(row, int(lens[i]), slot, window)
        got_clamped = hfv.frame_locate(row[:min(end, window)])
        got_whole = hfv.frame_locate(row[:end])
        assert got_whole == whole[:3] if whole[0] == 0 else got_whole == (whole[0], 0, 0), (names[i], i)
        if kind == "final":
            assert got_clamped == got_whole, (names[i], i, window)
        else:
            assert clamped[3][0] == "bound" and clamped[3][1] > window and end > window
            assert got_clamped[0] == clamped[0] and got_clamped[0] in (H.PARSE_ERROR, H.NOT_SCION), (names[i], i)
            assert hfv.frame_locate(row[:clamped[3][1] - 1])[0] == clamped[0]      # one byte short of the bound
            assert got_clamped[1:] == (0, 0)


@pytest.mark.parametrize("window", H.WINDOWS)
def test_placement_table(window):
    """Every class of the rule holds a frame at every window -- but "final ok" at 64, which no frame
    can reach: the shortest successful parse ends at byte 94 (frames_hostmem.MIN_OK_END), and that
    the corpus has none is asserted in its place."""
    frames, lens, _, _ = H.corpus()
    assert 300 <= len(frames) <= 900
    t = H.placement(frames, lens, window)
    print(window, t)
    for c in H.CLASSES[1:]:
        assert t[c] >= 1, (window, c, t)
    if window < H.MIN_OK_END:
        assert t[H.CLASSES[0]] == 0
    else:
        assert t[H.CLASSES[0]] >= 1, (window, t)
    assert H.retried(frames, lens, window).sum() == t[H.CLASSES[2]] + t[H.CLASSES[3]]
    assert H.retried(frames, lens, window)[-1]               # the last frame is undecided at every window
