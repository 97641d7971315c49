"""wrdec --batch=N: the partial decode of N consecutive segmented fields through one region-decode call writes, byte for byte,
the file that --batch=1 -- a call per field -- writes, with the same exit status."""
import os

import numpy as np
import pytest

from util import ROOT  # noqa: F401
from test_gpu_cli_seg import WRDEC, WRENC, parse_wrh, read, run
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

NX, NY, NZ = 28, 20, 24
FORMATS = ["wrs1", "ref", "wrs3", "wrs3", "wrs2"]  # of fields 0..4
ENCODERS = {"wrs1": "wrs1:seg=1008", "ref": "ref", "wrs3": "wrs3:strands=4:seg=1008", "wrs2": "wrs2:brick=8:seg=1008"}


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """A directory with data.wrh / data.wrb of five fields in the formats above: the same five fields coded once per format by
    wrenc, and record k taken from the run of its format."""
    src = tmp_path_factory.mktemp("src")
    with open(src / "data.bin", "wb") as fh:
        for k in range(5):
            fh.write(synth.field(NX, NY, NZ, seed=60 + k).tobytes())
    parts = {}
    for name, fmt in ENCODERS.items():
        d = tmp_path_factory.mktemp(name)
        os.symlink(src / "data.bin", d / "data.bin")
        r = run(WRENC, ["--format=" + fmt, "data.bin", "data.wrb", "data.wrh", "2", "0", "5", "2", str(NX), str(NY), str(NZ), "1e-5"], d)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        text = read(d / "data.wrh").decode()
        recs, lines, wrb = parse_wrh(text), text.split("\n"), read(d / "data.wrb")
        starts = [i for i, l in enumerate(lines) if l == " -----"] + [len(lines) - 1]
        ends = np.cumsum([r_["wrb_bytes"] for r_ in recs])
        parts[name] = dict(pre=lines[:starts[0]], rec=[lines[starts[k]:starts[k + 1]] for k in range(5)],
                           bytes=[wrb[int(e) - recs[k]["wrb_bytes"]:int(e)] for k, e in enumerate(ends)])
    out = tmp_path_factory.mktemp("mixed")
    with open(out / "data.wrh", "w") as fh:
        fh.write("\n".join(parts["wrs1"]["pre"] + [l for k, f in enumerate(FORMATS) for l in parts[f]["rec"][k]]) + "\n")
    with open(out / "data.wrb", "wb") as fh:
        fh.write(b"".join(parts[f]["bytes"][k] for k, f in enumerate(FORMATS)))
    sniff = [api.stream_sniff(np.frombuffer(parts[f]["bytes"][k], dtype=np.uint8)) for k, f in enumerate(FORMATS)]
    assert sniff[1] == 0 and all(v >= 1 for k, v in enumerate(sniff) if k != 1), sniff
    return out


def both(mixed, tmp_path, options, name):
    """(status, file bytes or None, stdout) of --batch=1 and of --batch=4"""
    out = []
    for batch in (1, 4):
        path = tmp_path / ("%s_b%d.bin" % (name, batch))
        r = run(WRDEC, options + ["--batch=%d" % batch, "data.wrb", "data.wrh", str(path), "2", "0"], mixed)
        out.append((r.returncode, read(path) if os.path.exists(path) else None, r.stdout))
    return out


@pytest.mark.parametrize("name,options", [("roi", ["--roi=3:20,0:20,10:11"]), ("level1", ["--level=1"]), ("planes1", ["--planes=1"]),
                                          ("roi_level2_planes1", ["--roi=1:6,0:5,2:3", "--level=2", "--planes=1"])])
def test_the_same_file_as_a_call_per_field(mixed, tmp_path, name, options):
    """All five fields selected: field 1, the reference's stream, is refused either way (status 1) and the four segmented
    fields are written -- 0 alone, then 2, 3, 4 through one call."""
    (rc1, f1, o1), (rc4, f4, o4) = both(mixed, tmp_path, options, name)
    assert rc1 == 1 and rc4 == 1, (o1[-1500:], o4[-1500:])
    assert "field 1" in o1 and "field 1" in o4
    assert f1 is not None and f4 is not None and f1 == f4
    for k in (0, 2, 3, 4):
        assert "partial decode, field %d" % k in o1 and "partial decode, field %d" % k in o4
    # the messages come in the order of the fields
    assert [l for l in o1.split("\n") if "field" in l] == [l for l in o4.split("\n") if "field" in l]


def test_single_fields(mixed, tmp_path):
    """--field=K: a group of one goes the way it goes today; the reference's field is refused as without --batch."""
    (rc1, f1, o1), (rc4, f4, o4) = both(mixed, tmp_path, ["--level=1", "--field=1"], "ref")
    assert rc1 == 1 and rc4 == 1 and f1 is None and f4 is None
    assert "not a segmented stream" in o1 and "not a segmented stream" in o4
    (rc1, f1, o1), (rc4, f4, o4) = both(mixed, tmp_path, ["--roi=0:28,0:20,0:24", "--field=3"], "one")
    assert rc1 == 0 and rc4 == 0 and f1 == f4 and len(f1) == 8 * NX * NY * NZ


def test_batch_option_refusals(mixed, tmp_path):
    for options in (["--batch=0", "--level=1"], ["--batch=x", "--level=1"], ["--batch=4"]):
        r = run(WRDEC, options + ["data.wrb", "data.wrh", str(tmp_path / "no.bin"), "2", "0"], mixed)
        assert r.returncode == 2 and not os.path.exists(tmp_path / "no.bin"), (options, r.stdout[-500:])
