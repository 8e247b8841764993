"""The launcher's plain single-Mandelbulb classification (rm_debug_bulb_plain, no GPU needed): which tables skip the object
transform, the ·scaleFactor and the Julia select in every evaluation.  The benchmark's tables must be among them."""
import ctypes as C
import os

import numpy as np

import helpers as h
from raymarcher_amd import abi, lib, scenes
from raymarcher_amd.render import Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plain(objs, n, g):
    return lib().rm_debug_bulb_plain(objs, n, C.byref(g))


def bulb(model=None, sf=1.0):
    return (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model, scale_factor=sf))


def test_headline_tables_are_the_plain_form():
    """scenes.mandelbulb and the scenefile through the loader: 1 on the diagonal, zeros of both signs elsewhere (the loader's
    inverse writes −0 into some entries), scaleFactor 1, power 8, no Julia seed."""
    for t in (scenes.mandelbulb(64, 36),
              Scene(path=os.path.join(ROOT, "tests", "golden", "scenes", "simple", "unit_mandelbulb.json")).tables(64, 36)):
        o = t.objects[0]
        inv = np.array(list(o.invModel), dtype=np.float32).reshape(4, 4)  # column-major: inv[c, r]
        assert (np.abs(inv) == np.eye(4, dtype=np.float32)).all()
        assert (np.diag(inv).view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
        assert np.float32(o.scaleFactor).view(np.uint32) == np.float32(1.0).view(np.uint32)
        assert t.globals_.power == 8.0 and tuple(t.globals_.juliaSeed) == (0.0, 0.0)
        assert plain(t.objects, t.num_objects, t.globals_) == 1


def test_every_other_form_is_general():
    g0 = h.make_globals()
    assert plain(bulb(), 1, g0) == 1
    o = bulb()
    for i in (1, 2, 4, 6, 8, 9, 12, 13, 14):                         # any zero of either sign off the diagonal
        o[0].invModel[i] = -0.0
    assert plain(o, 1, g0) == 1
    assert plain(bulb(), 1, h.make_globals(julia=(-0.0, 0.0))) == 1   # a zero seed of either sign: frag:782's length is 0
    assert plain(bulb(), 1, h.make_globals(julia=(0.35, -0.2))) == 0  # Julia
    assert plain(bulb(), 1, h.make_globals(julia=(0.0, 1e-30))) == 0  # (its squared length underflows: still general)
    assert plain(bulb(), 1, h.make_globals(power=6.0)) == 0           # power other than 8
    assert plain(bulb(h.translate(0.4, 0.0, 0.0)), 1, g0) == 0        # translated
    assert plain(bulb(h.rotation((0, 1, 0), 0.5)), 1, g0) == 0        # rotated
    assert plain(bulb(h.scale(2, 2, 2), 2.0), 1, g0) == 0             # scaled
    assert plain(bulb(h.scale(-1, 1, 1), 1.0), 1, g0) == 0            # mirrored: −1 on the diagonal
    assert plain(bulb(None, 0.5), 1, g0) == 0                         # identity transform, scaleFactor != 1
    o = bulb()
    o[0].invModel[3] = 5.0                                            # the fourth row is never read
    assert plain(o, 1, g0) == 1
    two = (abi.RmObject * 2)(h.make_object(abi.RM_MANDELBULB), h.make_object(abi.RM_SPHERE))
    assert plain(two, 2, g0) == 0                                     # the table walk
    assert plain((abi.RmObject * 1)(h.make_object(abi.RM_SPHERE)), 1, g0) == 0
    assert plain(None, 0, g0) == 0
    assert lib().rm_debug_bulb_plain(None, 1, C.byref(g0)) == -1
