"""Forged exposure stacks for the alignment tests (tests/test_align_host.py,
tests/test_gpu_align.py): random bytes (the shifts mean nothing, the contract still holds bit for
bit), identical frames, a flat frame (an empty eb), a frame all 0 beside a frame all 255, and the
planted-shift scene - at sizes that give L = 0, 0, 1, 1, 2, 3 and 4, odd sides at every level, row
widths that are no multiple of 32 or 64, and a frame beyond one tile in both directions with a
remainder."""
import functools

import numpy as np

import align_model

# (h, w): L = 0, 0, 1, 1, 2 below max_bits; 150 x 270 is capped by max_bits = 3, BIG by the default
SIZES = ((16, 16), (17, 33), (33, 40), (64, 48), (67, 129), (150, 270))
BIG = (301, 517)
MAX_BITS = {(150, 270): 3}          # (every other size: the default, 6)


def max_bits_of(h, w):
    return MAX_BITS.get((h, w), align_model.MAX_BITS)


def levels_of(h, w):
    return align_model.levels_for(h, w, max_bits_of(h, w))


def reach_of(h, w):
    """The largest shift the search can return."""
    return 2 ** (levels_of(h, w) + 1) - 1


def random_stack(h, w, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(k)]


def identical_stack(h, w, k, seed):
    return [random_stack(h, w, 1, seed)[0].copy() for _ in range(k)]


def flat_stack(h, w, k, seed):
    """Exposure 0 is one colour: its eb is empty and every count against it is 0."""
    stack = random_stack(h, w, k, seed)
    stack[0][:] = (40, 90, 200)
    return stack


def extremes_stack(h, w, k, seed):
    """Exposure 0 all 0, the last all 255, random bytes between them."""
    stack = random_stack(h, w, k, seed)
    stack[0][:] = 0
    stack[-1][:] = 255
    return stack


# ------------------------------------------------------------- the planted scene
GAIN_PAIRS = ((1.0, 1.0), (1.0, 0.25), (1.0, 2.0), (0.5, 2.0))    # (reference, other)


def radiance(h, w, seed):
    """A 64-fold horizontal ramp times the exponential of summed block noise at the scales 2, 4,
    8, 16 and 32 with sigma 0.35 each."""
    rng = np.random.default_rng(seed)
    x = np.arange(w, dtype=np.float64)[None, :]
    log = np.zeros((h, w))
    for scale in (2, 4, 8, 16, 32):
        coarse = 0.35 * rng.standard_normal((-(-h // scale), -(-w // scale)))
        log += np.repeat(np.repeat(coarse, scale, axis=0), scale, axis=1)[:h, :w]
    return 3.0 * 64.0 ** (x / max(w - 1, 1)) * np.exp(log)


def render(rad, gain, noise, rng):
    """The radiance at a gain, with unit Gaussian noise or without, as a grey BGR frame."""
    v = rad * gain + (rng.standard_normal(rad.shape) if noise else 0.0)
    return np.repeat(np.clip(np.rint(v), 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def offsets_of(h, w):
    """The planted (dx, dy) of a size: those of the list within the search's reach, and three with
    components of +- min(reach, min side // 8)."""
    reach = reach_of(h, w)
    big = min(reach, min(h, w) // 8)
    listed = [(0, 0), (1, 0), (-1, 0), (3, -2), (-5, 4)]
    out = [o for o in listed if max(abs(o[0]), abs(o[1])) <= reach]
    return out + [o for o in ((big, big), (-big, big), (big, -big)) if o not in out]


def planted_stack(h, w, offsets, gains=(1.0, 2.0), noise=True, seed=0, reference=0):
    """k = 1 + len(offsets) frames: the reference crop at gains[0], and one crop per planted
    (dx, dy) at gains[1].  aligned[y][x] = src[y - dy][x - dx] is the reference's view: the frame
    planted at (dx, dy) is the crop that starts dx to the right of and dy below the reference's."""
    margin = max([1] + [max(abs(dx), abs(dy)) for dx, dy in offsets])
    rad = radiance(h + 2 * margin, w + 2 * margin, seed)
    rng = np.random.default_rng(seed + 1)
    frames = []
    others = list(offsets)
    k = 1 + len(others)
    for e in range(k):
        if e == reference:
            dx, dy, gain = 0, 0, gains[0]
        else:
            (dx, dy), gain = others.pop(0), gains[1]
        crop = rad[margin + dy:margin + dy + h, margin + dx:margin + dx + w]
        frames.append(render(crop, gain, noise, rng))
    return frames


def recovery_cases():
    """(h, w, gains, noise, (dx, dy)) of the recovery test: every size, gain pair, noise choice and
    planted offset, but the ones the MODEL does not recover (listed in ``NOT_RECOVERED``, checked
    in tests/test_align_host.py)."""
    out = []
    for h, w in SIZES + (BIG,):
        for gains in GAIN_PAIRS:
            for noise in (False, True):
                for off in offsets_of(h, w):
                    case = (h, w, gains, noise, off)
                    if case not in NOT_RECOVERED:
                        out.append(case)
    return out


def _not_recovered():
    """The 32 of the 400 plants that the model misses (tests/test_align_host.py checks that it
    recovers every other one): 14 at 16 x 16, where dx = +1 moves a sixteenth of the frame out,
    and 18 of the 48 at the search's limit at the two largest sizes - a shift of 2^(L+1) - 1 is
    reached only if every level picks the outermost candidate."""
    same, dark, bright, wide = GAIN_PAIRS
    out = set()
    for gains, noise, offs in ((same, False, [(1, 0), (1, 1), (1, -1)]), (same, True, [(1, 0), (1, 1), (1, -1)]),
                               (bright, False, [(1, 0), (1, 1), (1, -1)]), (bright, True, [(1, 0), (1, 1), (1, -1)]),
                               (wide, False, [(1, 0), (1, -1)])):
        out |= {(16, 16, gains, noise, o) for o in offs}
    for noise in (False, True):
        out |= {(150, 270, same, noise, (15, 15)), (150, 270, dark, noise, (-15, 15)),
                (150, 270, bright, noise, (15, 15)),
                (301, 517, same, noise, (31, -31)), (301, 517, dark, noise, (-31, 31)),
                (301, 517, dark, noise, (31, -31)), (301, 517, bright, noise, (-31, 31)),
                (301, 517, bright, noise, (31, -31)), (301, 517, wide, noise, (31, -31))}
    return frozenset(out)


NOT_RECOVERED = _not_recovered()


def recovery_stack(case):
    h, w, gains, noise, off = case
    return planted_stack(h, w, [off], gains, noise, seed=h * 1000 + w)


# ------------------------------------------------------------------- the GPU cases
_MAKERS = {"random": random_stack, "identical": identical_stack, "flat": flat_stack,
           "extremes": extremes_stack}


def _cases():
    """(kind, h, w, k, reference): every size with random bytes, k = 2, 3 and 8 and the reference
    first, in the middle and last in turn; the other kinds on a few sizes."""
    cases = []
    for i, (h, w) in enumerate(SIZES + (BIG,)):
        k = (2, 3, 8)[i % 3]
        cases.append(("random", h, w, k, (0, k // 2, k - 1)[(i // 3 + i) % 3]))
    cases += [("identical", 33, 40, 3, 1), ("identical", 67, 129, 2, 0),
              ("flat", 17, 33, 2, 1), ("flat", 64, 48, 3, 0), ("flat", 150, 270, 3, 2),
              ("extremes", 16, 16, 2, 0), ("extremes", 67, 129, 3, 1),
              ("planted", 33, 40, 3, 1), ("planted", 64, 48, 2, 1), ("planted", 67, 129, 8, 7),
              ("planted", 150, 270, 3, 0), ("planted",) + BIG + (3, 1)]
    return cases


CASES = _cases()
IDS = [f"{kind}-{h}x{w}-k{k}r{r}" for kind, h, w, k, r in CASES]


# the planted (dx, dy) per frame of the planted cases, (0, 0) for the reference
PLANTED = {
    ("planted", 33, 40, 3, 1): [(3, -3), (0, 0), (-3, 3)],
    ("planted", 64, 48, 2, 1): [(3, -3), (0, 0)],
    ("planted", 67, 129, 8, 7): [(7, -7), (-7, 7), (7, 7), (-5, 4), (3, -2), (-1, 0), (1, 0), (0, 0)],
    ("planted", 150, 270, 3, 0): [(0, 0), (15, -15), (-15, 15)],
    ("planted",) + BIG + (3, 1): [(31, -31), (0, 0), (-5, 4)],
}


def planted_offsets(case):
    return list(PLANTED[case])


@functools.lru_cache(maxsize=None)
def stack_of(case):
    """The frames of a case (read-only arrays, made once)."""
    kind, h, w, k, r = case
    if kind == "planted":
        offs = planted_offsets(case)
        frames = planted_stack(h, w, offs[:r] + offs[r + 1:], (1.0, 2.0), True, 500 + CASES.index(case), r)
    else:
        frames = _MAKERS[kind](h, w, k, 2000 + CASES.index(case))
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def model_of(case):
    """The model's stages of a case, made once and shared."""
    _, h, w, _, r = case
    return align_model.stages(stack_of(case), r, max_bits_of(h, w))
