"""The solver handle's knob table (midagma_amd/csrc/solver_knobs.h: SolverKnobs, padded_dim),
built with g++ as a stand-alone program (tests/knobs/knobs_test.cpp; plain C++, no HIP header) and
run on the CPU: the experiments build reads every MIDAGMA_EXP_* variable into its own field, an
empty environment and the product build give the defaults (the "unset means follow the rule" states
included), the product object names no variable, and padded_dim follows midagma_create's rule."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "midagma_amd", "csrc")
SRC = os.path.join(REPO, "tests", "knobs", "knobs_test.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

# field: (variable, default, value set, field's value then).  The defaults are the ones the flat
# members' initialisers of the one-struct handle spelled: knob(NAME, dflt), !knob_set(NAME), and -1
# for "unset: follow the size rule" (AT_FOLD, COV_PAD_B2, COV_SPLIT, DATA_SPLIT).
KNOBS = {
    "no_fork": ("MIDAGMA_EXP_NO_FORK", 0, "1", 1),
    "no_small": ("MIDAGMA_EXP_NO_SMALL", 0, "0", 1),          # (set, whatever the value)
    "small_tcc": ("MIDAGMA_EXP_SMALL_TCC", 1, "0", 0),
    "nm_adapt": ("MIDAGMA_EXP_NM_ADAPT", 1, "0", 0),
    "cov_fork": ("MIDAGMA_EXP_COV_FORK", 0, "2", 2),
    "cov_la": ("MIDAGMA_EXP_COV_LA", 0, "1", 1),
    "eager": ("MIDAGMA_EXP_EAGER", 0, "1", 1),
    "data_flat_gj": ("MIDAGMA_EXP_DATA_FLAT_GJ", 0, "1", 1),
    "data_fork_fast": ("MIDAGMA_EXP_DATA_FORK_FAST", 1, "0", 0),
    "data_fast_rows": ("MIDAGMA_EXP_DATA_FAST_ROWS", 16384, "4096", 4096),
    "fast_group": ("MIDAGMA_EXP_FAST_GROUP", 4, "0", 1),      # (at least 1)
    "fuse_gemm": ("MIDAGMA_EXP_FUSE_GEMM", 1, "0", 0),
    "ctl_fold": ("MIDAGMA_EXP_CTL_FOLD", 1, "0", 0),
    "at_fold": ("MIDAGMA_EXP_AT_FOLD", -1, "0", 0),
    "build_resid0": ("MIDAGMA_EXP_BUILD_RESID0", 0, "1", 1),
    "cov_split": ("MIDAGMA_EXP_COV_SPLIT", -1, "3", 3),
    "cov_pad256": ("MIDAGMA_EXP_COV_PAD256", 1, "0", 0),
    "cov_pad_b2": ("MIDAGMA_EXP_COV_PAD_B2", -1, "1", 1),
    "gemm_ses": ("MIDAGMA_EXP_GEMM_SES", 0, "2", 2),
    "df": ("MIDAGMA_EXP_DF", 0, "1", 1),
    "df_per_cu": ("MIDAGMA_EXP_DF_PER_CU", 2, "1", 1),
    "tcc_fast_steps": ("MIDAGMA_EXP_TCC_FAST_STEPS", 5, "0", 0),
    "tcc_fix": ("MIDAGMA_EXP_TCC_FIX", 1, "0", 0),
    "tcc_fix_pre": ("MIDAGMA_EXP_TCC_FIX_PRE", 1, "3", 3),
    "tcc_fix_hold": ("MIDAGMA_EXP_TCC_FIX_HOLD", 8, "1", 1),
    "tcc_fix_easy": ("MIDAGMA_EXP_TCC_FIX_EASY", 0, "6", 6),
    "tcc_fastblk": ("MIDAGMA_EXP_TCC_FASTBLK", 1, "0", 0),
    "tcc_binv": ("MIDAGMA_EXP_TCC_BINV", 1, "2", 2),
    "prepad_mb": ("MIDAGMA_EXP_PREPAD_MB", 0, "96", 96),
    "sig_split": ("MIDAGMA_EXP_SIG_SPLIT", 1, "0", 0),
    "y_offset": ("MIDAGMA_EXP_Y_OFFSET", 0, "4096", 4096),
    "data_split": ("MIDAGMA_EXP_DATA_SPLIT", -1, "0", 0),    # (set to 0 is a value, not "unset")
    "xw_fullk": ("MIDAGMA_EXP_XW_FULLK", 0, "1", 1),
    "debug_handbacks": ("MIDAGMA_DEBUG_HANDBACKS", 0, "1", 1),
}
DEFAULTS = {f: v[1] for f, v in KNOBS.items()}

# midagma_create's rule: the next 64-multiple up to d = 192, 128-multiples above; cov mode pads
# 129 <= d <= 192 to 256 as well, and 256 < d <= 640 to a multiple of 256
DS = (64, 65, 128, 129, 192, 193, 256, 257, 640, 641, 1100)
PADDED = {
    "cov": dict(zip(DS, (64, 128, 128, 256, 256, 256, 256, 512, 768, 768, 1152))),
    "data": dict(zip(DS, (64, 128, 128, 192, 192, 256, 256, 384, 640, 768, 1152))),
}


def _build(tmp, name, *flags):
    exe = os.path.join(tmp, name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *flags, SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("knobs"))
    san = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    return {"exp": _build(tmp, "knobs_exp", "-DMIDAGMA_EXPERIMENTS"), "product": _build(tmp, "knobs_product"),
            "exp_san": _build(tmp, "knobs_exp_san", "-DMIDAGMA_EXPERIMENTS", *san),
            "product_san": _build(tmp, "knobs_product_san", *san), "tmp": tmp}


def _run(exe, env):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("MIDAGMA_")}, **env,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=") for line in r.stdout.split())
    fields = {k: int(v) for k, v in kv.items() if not k.startswith("D[")}
    dims = {(k[2:-1].split(",")[0], int(k[2:-1].split(",")[1])): int(v) for k, v in kv.items() if k.startswith("D[")}
    return fields, dims


ALL_SET = {v[0]: v[2] for v in KNOBS.values()}


@pytest.mark.parametrize("build", ["exp", "exp_san"])
def test_empty_environment_gives_the_defaults(programs, build):
    fields, _ = _run(programs[build], {})
    assert fields == DEFAULTS


@pytest.mark.parametrize("build", ["product", "product_san"])
def test_product_build_reads_no_variable(programs, build):
    for env in ({}, ALL_SET):
        fields, dims = _run(programs[build], env)
        assert fields == DEFAULTS
        assert dims == {(m, d): D for m, tab in PADDED.items() for d, D in tab.items()}


def test_product_object_names_no_variable(programs):
    obj = os.path.join(programs["tmp"], "knobs_product.o")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, "-c", SRC, "-o", obj], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr
    for path in (obj, programs["product"]):
        blob = open(path, "rb").read()
        assert b"MIDAGMA_EXP_" not in blob and b"MIDAGMA_DEBUG_HANDBACKS" not in blob, path


@pytest.mark.parametrize("field", sorted(KNOBS))
def test_each_variable_sets_its_field_alone(programs, field):
    var, _, text, value = KNOBS[field]
    fields, _ = _run(programs["exp"], {var: text})
    assert fields == dict(DEFAULTS, **{field: value})


def test_every_variable_set(programs):
    fields, _ = _run(programs["exp_san"], ALL_SET)
    assert fields == {f: v[3] for f, v in KNOBS.items()}


def test_padded_dim_rule(programs):
    _, dims = _run(programs["exp"], {})
    assert dims == {(m, d): D for m, tab in PADDED.items() for d, D in tab.items()}
    # COV_PAD256 = 0: cov keeps 129..192 at 192; data mode never looks at it
    _, dims = _run(programs["exp"], {"MIDAGMA_EXP_COV_PAD256": "0"})
    assert dims == {(m, d): 192 if (m, d) in (("cov", 129), ("cov", 192)) else D for m, tab in PADDED.items()
                    for d, D in tab.items()}
    # COV_PAD_B2 = 0: never a 256-multiple; 1: at every d > 256
    _, dims = _run(programs["exp"], {"MIDAGMA_EXP_COV_PAD_B2": "0"})
    assert [dims[("cov", d)] for d in (257, 640, 641, 1100)] == [384, 640, 768, 1152]
    _, dims = _run(programs["exp"], {"MIDAGMA_EXP_COV_PAD_B2": "1"})
    assert [dims[("cov", d)] for d in (256, 257, 640, 641, 1100)] == [256, 512, 768, 768, 1280]
    assert [dims[("data", d)] for d in DS] == [PADDED["data"][d] for d in DS]
