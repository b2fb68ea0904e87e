"""The ray kernel forms one cubic B-spline basis element per lane without forming the other three (basis1 in rays.hip).  That the
per-lane form gives the bits of the plain form -- four numerators, one selected, inv/CalSurfG.f90:2145-2148 -- is a property of fp32
arithmetic that tools/check_basis.c verifies by brute force (stride 1 = all 2^32 floats for i = 0..3, 0 mismatches:
profiles/rays_step_cut.md).  Here: every 193rd bit pattern plus zeros, denormals, infinities and NaNs, a second of one core."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _body(text, name):
    """the statements of function `name`, white space removed"""
    m = re.search(r"float " + name + r"\(float v, int i\) \{(.*?)\n\}", text, re.S)
    assert m, name
    return re.sub(r"\s+", "", m.group(1))


def test_checked_form_is_the_kernel_source():
    kernel = _body(open(os.path.join(ROOT, "dazimsurftomo_amd", "csrc", "rays.hip")).read(), "basis1")
    checked = _body(open(os.path.join(ROOT, "tools", "check_basis.c")).read(), "lane_num")
    assert kernel.replace("returndiv6((i==0||i==3)?t3:n);", "return(i==0||i==3)?t3:n;") == checked


def test_per_lane_basis_equals_the_plain_form(tmp_path):
    exe = str(tmp_path / "check_basis")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "check_basis.c"), "-lm"])
    p = subprocess.run([exe, "193"], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and " 0 mismatches" in p.stdout, p.stdout
    assert int(p.stdout.split(" of ")[1].split()[0]) > 2 ** 32 // 193
