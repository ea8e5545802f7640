"""Scenes whose materials, lights and ambient leave the ranges every other test keeps to
(reflectivity in [0, 1], colours in [0, 1), shininess in [0.01, 2000]), with the oracle's answers:

  CASES       twelve named variants of one scene of five spheres and two lights: reflectivity above 1 and
              below 0, negative and over-unit colours, lights and ambient, and shininess that is negative,
              zero, tiny, at the edges of the device's integer and double-double pow domains, or beyond them
  F64_CASES   five more whose shininess values are all 0 or 1 (no pow rounding at all: pow(x, 1) is x and
              pow(x, 0) is 1) or all -1, for the unquantised framebuffers
  PATH_CASES  the three whose reflectivities decide `reflectivity > 0` (main.cpp:43) near and beyond zero
  text(case, form)   "dense": the five spheres; "sparse": 40 small spheres on a lattice before the same
              camera, sphere i with the case's material A, B or C by i % 3, so that a wave holds only a few
              hit lanes (the lights-over-helper-lanes pass of the render kernels)

Tags: `exact` (every shininess is 0, 1 or a whole number in [1, 1024]: the device's pow is the oracle's, so
RGB8 is byte-identical) or pm1 (anything else: each channel within 1), `expects_negative` (the oracle counts
channels quantised below 0 at every size, depth and form listed), `has_inf` (negative shininess at
rdv == 0: pow(+0, y < 0) = +inf channels).  Negative shininess is never combined with a negative or zero
light or ambient channel or reflectivity >= 1: 0 * inf and inf - inf are NaN, and (int)NaN is undefined in
the reference.

Shared by test_material_cases_host.py (which pins the oracle to the reference on these texts and asserts
the tags' conditions on the oracle's fp64 framebuffer) and test_gpu_materials.py.  Every oracle result is
computed once per process and never modified."""
import functools

GROUND = "sphere 0 -1001 -8 1000 0.6 0.6 0.6 0.2 0.5 %s"
MIRROR = "sphere 0 2.1 -9 1 0.9 0.9 0.9 1.0 0.5 %s"
CAMERA = "camera 0 1 2 0 0 -8 55"
CENTRES = ("-2.2 0 -8", "0 0 -8", "2.2 0 -8")  # A, B, C: unit spheres

# colour / reflectivity / shininess of A, B, C, the lights (colour and intensity) and the ambient
DEFAULT = {
    "colour": ("0.9 0.2 0.2", "0.2 0.9 0.2", "0.2 0.2 0.9"),
    "refl": ("0.3", "0.0", "0.7"),
    "shin": ("20", "5", "100"),
    "shin_ground": "20",
    "shin_mirror": "50",
    "lights": ("1 1 1 1", "0.6 0.5 0.4 1"),
    "ambient": "0.1 0.1 0.1",
}
LIGHT_POSITIONS = ("5 8 0", "-6 4 -2")

CASES = {
    "refl_above_one": {"refl": ("1.5", "0.0", "2.5")},
    "refl_negative": {"refl": ("-0.5", "-2", "-1e-300")},
    "colour_negative": {"colour": ("-0.9 0.2 -0.2", "0.2 -0.9 0.2", "-1 -1 -1")},
    "colour_large": {"colour": ("40 0.2 0.2", "0.2 300 0.2", "2 2 2")},
    "light_negative": {"lights": ("-1 -0.5 0.25 1", "0.6 -2 0.4 1")},
    "light_large": {"lights": ("1000 0 1e6 1", "0.6 0.5 0.4 1")},
    "ambient_negative": {"ambient": "-0.5 0.2 -1e-3"},
    "shin_negative": {"shin": ("-2", "-0.5", "-40"), "refl": ("0.3", "0.0", "0.5")},
    "shin_zero_tiny": {"shin": ("0", "1e-300", "-0")},
    "shin_int_edges": {"shin": ("1024", "1025", "65536")},
    "shin_huge": {"shin": ("65537", "1e9", "1e300")},
    "shin_frac_edges": {"shin": ("1023.5", "0.999999999", "65535.5")},
}
_S01 = {"shin": ("1", "0", "1"), "shin_ground": "1", "shin_mirror": "0"}
F64_CASES = {
    "refl_above_one_s01": dict(CASES["refl_above_one"], **_S01),
    "colour_negative_s01": dict(CASES["colour_negative"], **_S01),
    "light_negative_s01": dict(CASES["light_negative"], **_S01),
    "ambient_negative_s01": dict(CASES["ambient_negative"], **_S01),
    # the mirror (reflectivity 1) keeps a shininess of 1: (1 - 1) * inf is NaN
    "shin_minus_one": {"shin": ("-1", "-1", "-1"), "shin_ground": "-1", "shin_mirror": "1",
                       "refl": ("0.3", "0.0", "0.5")},
}
PATH_CASES = {
    "refl_negative": CASES["refl_negative"],
    "refl_above_one": CASES["refl_above_one"],
    "refl_zeros": {"refl": ("-0", "0", "1e-300")},
}
ALL_CASES = {**CASES, **F64_CASES, **PATH_CASES}

NAMES = tuple(CASES)
EXPECTS_NEGATIVE = ("refl_above_one", "colour_negative", "light_negative", "ambient_negative")
HAS_INF = ("shin_negative", "shin_minus_one")
F64_EXPECTS_NEGATIVE = tuple(n + "_s01" for n in EXPECTS_NEGATIVE)

SIZES = ((64, 48), (97, 61))
DEPTHS = {"dense": (1, 4, 10), "sparse": (1, 4)}
FORMS = ("dense", "sparse")
# sizes of a case's sparse form: a case whose sparse form had no negative channel at a size would drop that
# size here (none does at the lattice below)
SPARSE_SIZES = {name: SIZES for name in NAMES}
F64_SHAPE = (97, 61, 4)   # the unquantised tile framebuffers (F64_CASES, dense)
PATH_SHAPE = (64, 48, 4)  # the path queries (PATH_CASES, dense)
AA_CASES = EXPECTS_NEGATIVE + ("shin_negative",)
# the 4-sample antialias renders (AA_CASES, dense).  Averaging four samples leaves refl_above_one no channel
# below 0 at depth 4 (it has two in one-sample mode), so depth 1 is rendered as well: there it has some.
AA_SHAPES = ((64, 48, 4), (64, 48, 1))
AA_NO_NEGATIVE = (("refl_above_one", (64, 48, 4)),)

# the lattice of the sparse form: 8 x 5 spheres at z = -8
LATTICE_NX, LATTICE_NY, LATTICE_STEP, LATTICE_RADIUS = 8, 5, 0.75, 0.3


def _fields(case):
    f = dict(DEFAULT)
    f.update(ALL_CASES[case])
    return f


def _whole(s):
    v = float(s)
    return v == 0.0 or (v == int(v) and 1.0 <= v <= 1024.0)


def is_exact(case):
    """Every shininess of the case's spheres (both forms) is 0, 1 or a whole number in [1, 1024]."""
    f = _fields(case)
    return all(_whole(s) for s in f["shin"] + (f["shin_ground"], f["shin_mirror"]))


def expects_negative(case):
    return case in EXPECTS_NEGATIVE or case in F64_EXPECTS_NEGATIVE


def has_inf(case):
    return case in HAS_INF


def sizes(case, form):
    return SPARSE_SIZES[case] if form == "sparse" and case in SPARSE_SIZES else SIZES


def combos(case, form):
    """The (W, H, depth) the GPU tests render this case's form at."""
    return [(W, H, D) for W, H in sizes(case, form) for D in DEPTHS[form]]


def used():
    """Every (case, form, W, H, depth) the GPU tests render in one-sample mode."""
    out = [(c, f, W, H, D) for c in NAMES for f in FORMS for W, H, D in combos(c, f)]
    out += [(c, "dense") + F64_SHAPE for c in F64_CASES]
    out += [(c, "dense") + PATH_SHAPE for c in PATH_CASES if c not in CASES]
    return out


@functools.lru_cache(maxsize=None)
def text(case, form="dense"):
    f = _fields(case)
    lines = []
    if form == "dense":
        lines.append(GROUND % f["shin_ground"])
        for k in range(3):
            lines.append("sphere %s 1 %s %s 0.5 %s" % (CENTRES[k], f["colour"][k], f["refl"][k], f["shin"][k]))
        lines.append(MIRROR % f["shin_mirror"])
    else:
        i = 0
        for iy in range(LATTICE_NY):
            for ix in range(LATTICE_NX):
                x = (ix - 0.5 * (LATTICE_NX - 1)) * LATTICE_STEP
                y = (iy - 0.5 * (LATTICE_NY - 1)) * LATTICE_STEP + 0.2
                k = i % 3
                lines.append("sphere %r %r -8 %r %s %s 0.5 %s" % (x, y, LATTICE_RADIUS, f["colour"][k], f["refl"][k],
                                                                 f["shin"][k]))
                i += 1
    for pos, col in zip(LIGHT_POSITIONS, f["lights"]):
        lines.append("light %s %s" % (pos, col))
    lines.append("ambient " + f["ambient"])
    lines.append(CAMERA)
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def oracle(case, form, W, H, depth):
    """(rgb bytes, counts dict, fp64 framebuffer in PPM row order as a read-only numpy [H, W, 3]) of the
    oracle's one-frame render."""
    import numpy as np
    import orc

    rgb, counts, _, fb = orc.OracleScene(text=text(case, form)).render(W, H, depth, threads=4, want_fb=True)
    fb = np.array(fb, np.float64).reshape(H, W, 3)
    fb.setflags(write=False)
    return rgb, counts, fb


@functools.lru_cache(maxsize=None)
def oracle_aa(case, W, H, depth):
    """(rgb bytes, counts dict, fp64 framebuffer) of the oracle's 4-sample antialias render of the dense form."""
    import numpy as np
    import orc

    rgb, counts, _, fb = orc.OracleScene(text=text(case, "dense")).render_aa(W, H, depth, samples=4, threads=4,
                                                                              want_fb=True)
    fb = np.array(fb, np.float64).reshape(H, W, 3)
    fb.setflags(write=False)
    return rgb, counts, fb


def ray_counts(counts):
    return (counts["primary"], counts["shadow"], counts["reflect"])
