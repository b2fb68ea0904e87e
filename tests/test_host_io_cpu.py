"""The host programs' shared readers and writers (host/dazim_io.f90) on the CPU: the module and tests/host_io_driver.f90 are
compiled with flang into the temporary directory and run there; no GPU and no HIP library are involved.  Every check is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = shutil.which("flang") or "/opt/rocm/lib/llvm/bin/flang"

pytestmark = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not found (PATH, /opt/rocm/lib/llvm/bin)")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_io_build")
    for src in (os.path.join(ROOT, "host", "dazim_io.f90"), os.path.join(ROOT, "tests", "host_io_driver.f90")):
        obj = os.path.splitext(os.path.basename(src))[0] + ".o"
        subprocess.check_call([FLANG, "-O2", "-ffp-contract=off", "-c", src, "-o", obj], cwd=d)
    subprocess.check_call([FLANG, "-o", "host_io_driver", "host_io_driver.o", "dazim_io.o"], cwd=d)
    return str(d / "host_io_driver")


def golden(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return {k: str(g[k]) for k in g.keys()}


def workdir(d, g, *outs):
    d.mkdir(exist_ok=True)
    for k in ("in:para.in", "in:MOD", "in:surf_synth.dat") + tuple("out:" + o for o in outs):
        (d / k.split(":", 1)[1]).write_text(g[k])
    return d


def run(driver, d, *args):
    return subprocess.run([driver, *args], cwd=d, timeout=120, capture_output=True, text=True)


def same_text(a, b):
    """equal byte for byte, at most one trailing newline aside"""
    strip = lambda s: s[:-1] if s.endswith("\n") else s
    return strip(a) == strip(b)


@pytest.mark.parametrize("name", ["program_joint", "program_iso"])
def test_reference_files_pass_through_unchanged(driver, tmp_path, name):
    """MOD_Ref, DSurfTomo.inv and phaseV_FWD.dat as the reference program wrote them, read with read_mod / read_map and written
    back with write_mod, write_vs_model and write_phase_map"""
    g = golden(name)
    d = workdir(tmp_path, g, "MOD_Ref", "phaseV_FWD.dat")
    out = run(driver, d, "roundtrip")
    assert out.returncode == 0, out.stdout + out.stderr
    assert " read phaseV_FWD.dat" in out.stdout.splitlines() and " read phaseV_FWD.dat" in (d / "driver.log").read_text().splitlines()
    for ours, theirs, nlines in (("MOD_out", "MOD_Ref", 86), ("DSurfTomo_out.inv", "DSurfTomo.inv", 1275), ("phaseV_out.dat", "phaseV_FWD.dat", 975)):
        assert len(g["out:" + theirs].splitlines()) == nlines
        assert same_text((d / ours).read_text(), g["out:" + theirs]), theirs


@pytest.mark.parametrize("name", ["program_joint", "program_iso"])
def test_read_data_counts(driver, tmp_path, name):
    """the number of data is the one the reference program reports; sources and receivers per period as a plain parse of the file"""
    g = golden(name)
    out = run(driver, workdir(tmp_path, g), "data")
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == " begin load data file....."
    reported = [line for line in g["out:__stdout__"].splitlines() if "Number of all measurements" in line]
    assert len(reported) == 1 and lines[1] == reported[0]
    nsrc, nrc = {}, {}
    for line in g["in:surf_synth.dat"].splitlines():
        if line.startswith("#"):
            k = int(line.split()[3])
            nsrc[k] = nsrc.get(k, 0) + 1
        elif line.strip():
            nrc[k] = nrc.get(k, 0) + 1
    assert lines[2].split() == ["dall", str(sum(nrc.values()))] and int(reported[0].split()[-1]) == sum(nrc.values())
    kmax = 5
    assert [line.split() for line in lines[3:]] == [["period", str(k), str(nsrc.get(k, 0)), str(nrc.get(k, 0))] for k in range(1, kmax + 1)]


def test_read_map_checks_the_file_against_para_in(driver, tmp_path):
    """a missing file, a line too few or too many, a wrong period and a coordinate 2e-3 degrees off the inner grid are refused with
    read_map's messages and a non-zero status; a coordinate 5e-4 degrees off is accepted (the tolerance is 1e-3)"""
    g = golden("program_joint")
    d = workdir(tmp_path, g)
    lines = g["out:phaseV_FWD.dat"].splitlines()
    assert len(lines) == 975

    def edited(i, col, delta):
        v = [float(x) for x in lines[i].split()]
        v[col] += delta
        return lines[:i] + ["%10.4f%10.4f%10.4f%10.4f" % tuple(v)] + lines[i + 1:]

    cases = {
        "good.dat": (lines, None),
        "short.dat": (lines[:-1], "has fewer lines than para.in's inner grid times its periods"),
        "long.dat": (lines + lines[-1:], "has more lines than para.in's inner grid times its periods"),
        "period.dat": (edited(400, 2, 1.0), "its periods differ from para.in's"),
        "lon_off.dat": (edited(17, 0, 2e-3), "its coordinates are not para.in's inner grid at"),
        "lat_off.dat": (edited(17, 1, -2e-3), "its coordinates are not para.in's inner grid at"),
        "lon_near.dat": (edited(17, 0, 5e-4), None),
        "lat_near.dat": (edited(17, 1, -5e-4), None),
    }
    for fname, (text, message) in cases.items():
        (d / fname).write_text("\n".join(text) + "\n")
        out = run(driver, d, "map", fname)
        if message is None:
            assert out.returncode == 0 and out.stdout.splitlines() == ["map ok"], (fname, out.stdout, out.stderr)
        else:
            assert out.returncode != 0 and "map ok" not in out.stdout, (fname, out.stdout)
            assert out.stdout.startswith(" ERROR: " + fname) and message in out.stdout, (fname, out.stdout)
            assert "a map file does not match para.in" in out.stderr, (fname, out.stderr)
    out = run(driver, d, "map", "absent.dat")
    assert out.returncode != 0 and out.stdout.startswith(" ERROR: absent.dat is missing (SurfPhaseMaps_amd writes it)"), out.stdout
    assert "a map file is missing" in out.stderr


def test_optional_argument_parser(driver, tmp_path):
    """text that is not a number is refused with the Monte-Carlo program's message and a non-zero status"""
    d = workdir(tmp_path, golden("program_joint"))
    out = run(driver, d, "arg", "abc")
    assert out.returncode != 0 and out.stdout.splitlines() == [" ERROR: argument 2 is not a number: abc"], out.stdout
    assert "bad argument" in out.stderr
    out = run(driver, d, "arg", "1e-2")
    assert out.returncode == 0 and np.float32(out.stdout.split()[1]) == np.float32(1e-2), out.stdout
    out = run(driver, d, "arg")
    assert out.returncode == 0 and float(out.stdout.split()[1]) == 0.5, out.stdout
