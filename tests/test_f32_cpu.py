"""fp32 entry points without a GPU: the library exports them and the header declares them; the command-line tools, linked
against a codec without them (the reference's libwaverange, or the oracle under its ABI), take the widening path through
their weak references and still write the reference's fp32 files."""
import os
import re
import shutil
import subprocess

import pytest

from util import ROOT, build_cli, codec_library

F32_SYMBOLS = ("wr_encode_host_f32", "wr_decode_host_f32", "wr_decode_finish_host_f32", "wr_encoding_wrap_f32", "wr_decoding_wrap_f32")
LIB = os.path.join(ROOT, "waverange_amd", "libwaverange_amd.so")


def dynamic_symbols(path, kind):
    out = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
    return {parts[-1] for parts in (line.split() for line in out.splitlines()) if len(parts) >= 2 and parts[-2] == kind}


@pytest.mark.skipif(shutil.which("nm") is None, reason="no nm")
def test_library_exports_the_f32_entry_points():
    if not os.path.exists(LIB):
        from waverange_amd import build
        build.build(verbose=False)
    exported = dynamic_symbols(LIB, "T")
    for name in F32_SYMBOLS:
        assert name in exported, name


def test_header_declares_the_f32_entry_points():
    with open(os.path.join(ROOT, "include", "waverange_amd.h")) as fh:
        text = fh.read()
    for name in F32_SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\(", text), name


@pytest.fixture(scope="module")
def cli_without_f32(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_f32"))
    so = codec_library()
    assert not set(F32_SYMBOLS) & dynamic_symbols(so, "T"), "the codec under test must not have the fp32 entry points"
    return build_cli("wrenc", so, d), build_cli("wrdec", so, d)


@pytest.mark.skipif(shutil.which("nm") is None, reason="no nm")
@pytest.mark.parametrize("case", ["argv_two_fp32", "inmeta_new_type0", "inmeta_old_type1_bigendian"])
def test_cli_fp32_cases_through_the_weak_fallback(case, cli_without_f32):
    import json
    from test_cli import run_case
    wrenc, wrdec = cli_without_f32
    assert "wr_encoding_wrap_f32" in dynamic_symbols(wrenc, "w"), "wrenc must refer to the fp32 encoder weakly"
    assert "wr_decoding_wrap_f32" in dynamic_symbols(wrdec, "w"), "wrdec must refer to the fp32 decoder weakly"
    with open(os.path.join(ROOT, "tests", "golden", "cli.json")) as fh:
        g = json.load(fh)[case]
    run_case(case, wrenc, wrdec, g)
