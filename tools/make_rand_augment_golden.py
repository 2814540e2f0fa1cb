"""Records tests/golden/rand_augment_contract.json from the UNMODIFIED reference's slowfast/datasets/rand_augment.py
(``AugmentOp``, ``rand_augment_transform``).  Build container only (needs the reference tree and Pillow).

    python tools/make_rand_augment_golden.py

The reference file imports only PIL and numpy and is loaded BY FILE PATH.  Every clip has T = 3 frames drawn from a seeded
generator with a different range per frame and per channel (tests/rand_augment_checks.py:case_frames draws them again), so a
statistic of the clip differs from one of a frame.

* op cases: ``AugmentOp(name, prob=1.0, magnitude=m, hparams={"interpolation": filter})`` on a landscape 18 x 26 and a portrait
  26 x 18 clip -- the 15 ops of the increasing set and the plain variants that differ; geometric ops with both signs and both
  filters, enhance ops with a factor below and above 1, Posterize bits 0 and 4, Solarize thresholds 256 and 0, Equalize and
  AutoContrast once more on a clip with one constant channel.  ``random`` is seeded in front of every call so that the level
  function's sign draw is the wanted one.
* whole-transform cases: ``rand_augment_transform(config, {"interpolation": filter})`` as create_random_augment calls it, three
  samples of different sizes under one seed of ``np.random`` and ``random``.  The seeds are found by search: over these cases
  every one of the 15 ops is applied and at least one op is skipped by its probability draw.

Per case the fixture keeps ``rows`` (per sample and layer: op code, skipped, argument -- captured by wrapping the reference
``AugmentOp.__call__`` and, inside it, the level and image functions while they run), ``magnitudes`` (the clipped magnitude the level function received, null
where the op has none), ``np_after`` / ``py_after`` (one more ``np.random.uniform()`` / ``random.random()``: how far each
generator got), the reference's output -- ``out`` (PIL's bytes, sample after sample, base64) for the whole-transform cases,
``sha256`` (the digest of every sample's bytes) for the op cases, whose 96 clips would otherwise make half a megabyte of
fixture -- and ``effect_diff``: by how many bytes that output differs
from the input and from four deliberately wrong variants of the restatement in tests/rand_augment_checks.py (bicubic with
a = -0.5, rounding instead of truncating, the histogram over the clip instead of the frame, the sharpness border one pixel
further in).  The restatement WITHOUT a variant must reproduce the reference byte for byte, and a variant an op case can tell
apart must change at least one byte.  Recorded results only: no reference program text goes into the fixture or this tool.
"""
import base64
import importlib.util
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("SLOWFAST_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "rand_augment_contract.json")
sys.path.insert(0, ROOT)

LAND, PORT, SQUARE = (18, 26), (26, 18), (26, 26)
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
SIGNED = GEOMETRIC + ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing")


def load_reference():
    path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", "rand_augment.py")
    spec = importlib.util.spec_from_file_location("reference_rand_augment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def op_cases():
    """(name, reference op name, magnitude, interpolation, negative sign wanted or None, constant channel or None)"""
    cases = []
    for name in GEOMETRIC:
        for interp in ("bicubic", "bilinear"):
            for neg in (False, True):
                cases.append(("%s %s %s" % (name, interp, "negative" if neg else "positive"), name, 7, interp, neg, None))
    for name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        for neg in (True, False):
            cases.append(("%s factor %s 1" % (name, "below" if neg else "above"), name, 6, "bicubic", neg, None))
    for name in ("Color", "Contrast", "Brightness", "Sharpness"):
        for m in (2, 9):
            cases.append(("%s magnitude %d" % (name, m), name, m, "bicubic", None, None))
    for name in ("AutoContrast", "Equalize"):
        cases.append((name, name, 5, "bicubic", None, None))
        cases.append((name + ", one constant channel", name, 5, "bicubic", None, 1))
    cases.append(("Invert", "Invert", 5, "bicubic", None, None))
    cases.append(("PosterizeIncreasing bits 0", "PosterizeIncreasing", 10, "bicubic", None, None))
    cases.append(("PosterizeIncreasing bits 4", "PosterizeIncreasing", 0, "bicubic", None, None))
    cases.append(("Posterize bits 2", "Posterize", 5, "bicubic", None, None))
    cases.append(("SolarizeIncreasing threshold 256", "SolarizeIncreasing", 0, "bicubic", None, None))
    cases.append(("SolarizeIncreasing threshold 0", "SolarizeIncreasing", 10, "bicubic", None, None))
    cases.append(("Solarize threshold 128", "Solarize", 5, "bicubic", None, None))
    cases.append(("SolarizeAdd 55", "SolarizeAdd", 5, "bicubic", None, None))
    return cases


TRANSFORM_CASES = [("rand-m7-n4-mstd0.5-inc1", "bicubic"), ("rand-m9-mstd0.5-inc1", "bicubic"), ("rand-m9-n2-w0", "bilinear")]


def main():
    from PIL import Image
    from slowfast_amd import rand_augment as ra
    from tests import rand_augment_checks as checks
    ref = load_reference()
    T = 3
    checks.T = T
    code = {}
    for names in (ref._RAND_TRANSFORMS, ref._RAND_INCREASING_TRANSFORMS):
        for i, n in enumerate(names):
            code[n] = i
    assert [ref._RAND_TRANSFORMS[i] for i in range(15)] == list(ra.OP_NAMES)
    pil_filter = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}

    def to_images(frames):
        return [Image.fromarray(f, "RGB") for f in frames.numpy()]

    def to_bytes(images):
        return np.stack([np.asarray(im) for im in images])

    class Recording:
        """While active, every ``AugmentOp.__call__`` of the reference files [op code, skipped, argument] in ``rows`` and the
        clipped magnitude its level function received (None: no level function, or skipped) in ``magnitudes``."""

        def __init__(self, code_of):
            self.code_of, self.rows, self.magnitudes = code_of, [], []

        def __enter__(self):
            rec, call = self, ref.AugmentOp.__call__
            self.call = call

            def recording_call(op, img_list):
                seen = {}
                level_fn, aug_fn = op.level_fn, op.aug_fn
                if level_fn is not None:
                    def level(magnitude, hparams):
                        args = level_fn(magnitude, hparams)
                        seen["magnitude"], seen["arg"] = float(magnitude), float(args[0])
                        return args
                    op.level_fn = level

                def aug(img, *args, **kwargs):
                    seen["applied"] = True
                    return aug_fn(img, *args, **kwargs)
                op.aug_fn = aug
                try:
                    res = call(op, img_list)
                finally:
                    op.level_fn, op.aug_fn = level_fn, aug_fn
                applied = bool(seen.get("applied"))
                rec.rows.append([rec.code_of[id(op)], not applied, seen.get("arg", 0.0) if applied else 0.0])
                rec.magnitudes.append(seen.get("magnitude"))
                return res
            ref.AugmentOp.__call__ = recording_call
            return self

        def __exit__(self, *exc):
            ref.AugmentOp.__call__ = self.call

    def effects(case, frames, outs):
        table = checks.case_table(case)
        exact = checks.restate_batch(frames, table)
        assert all(checks.differing(a, b) == 0 for a, b in zip(exact, outs)), ("the restatement differs from PIL", case["name"])
        eff = {"input": sum(checks.differing(f, o) for f, o in zip(frames, outs))}
        for v in checks.VARIANTS:
            eff[v] = sum(checks.differing(a, o) for a, o in zip(checks.restate_batch(frames, table, v), outs))
        return eff

    cases = []
    for k, (name, ref_name, magnitude, interp, neg, const) in enumerate(op_cases()):
        sizes = [LAND, PORT]
        data_seed = 1000 + k
        frames = checks.case_frames(data_seed, sizes, const)
        seed = None
        if ref_name in SIGNED:
            seed = next(s for s in range(1000) if (random.seed(s), random.random() > 0.5)[1] == bool(neg))
        rows, mags, outs = [], [], []
        for f in frames:
            op = ref.AugmentOp(ref_name, prob=1.0, magnitude=magnitude, hparams={"interpolation": pil_filter[interp]})
            if seed is not None:
                random.seed(seed)
            with Recording({id(op): code[ref_name]}) as rec:
                outs.append(to_bytes(op(to_images(f))))
            assert len(rec.rows) == 1 and not rec.rows[0][1]
            rows.append(rec.rows)
            mags.append(rec.magnitudes)
        case = dict(kind="op", name=name, reference_op=ref_name, interpolation=interp, sizes=sizes, data_seed=data_seed,
                    rows=rows, magnitudes=mags)
        if const is not None:
            case["constant_channel"] = const
        case["effect_diff"] = effects(case, frames, outs)
        eff, c = case["effect_diff"], code[ref_name]
        identity = ref_name.startswith("Solarize") and rows[0][0][2] == 256
        assert (eff["input"] > 0) != identity, (name, eff)
        if c in ra.AFFINE_OPS:
            assert eff["round"] > 0 and (interp != "bicubic" or eff["cubic_half"] > 0), (name, eff)
            assert (rows[0][0][2] < 0) == bool(neg)
        if c in ra.HIST_OPS:
            assert eff["clip_hist"] > 0, (name, eff)
        if c == ra.SHARPNESS:
            assert eff["sharp_border"] > 0, (name, eff)
        if c in ra.ENHANCE_OPS and neg is not None:
            assert (rows[0][0][2] < 1) == bool(neg)
        case["sha256"] = [checks.digest(o) for o in outs]
        cases.append(case)

    def run_transform(config, interp, seed, sizes, data_seed):
        frames = checks.case_frames(data_seed, sizes)
        np.random.seed(seed)
        random.seed(seed)
        rows, mags, outs = [], [], []
        for f in frames:                                    # a transform per clip, as the loader builds it
            tf = ref.rand_augment_transform(config, {"translate_const": 8, "interpolation": pil_filter[interp]})
            with Recording({id(op): i for i, op in enumerate(tf.ops)}) as rec:
                outs.append(to_bytes(tf(to_images(f))))
            rows.append(rec.rows)
            mags.append(rec.magnitudes)
        return frames, rows, mags, outs, float(np.random.uniform()), random.random()

    covered, skipped = set(), False
    chosen = []
    for k, (config, interp) in enumerate(TRANSFORM_CASES):
        sizes = [LAND, PORT, SQUARE]
        best = None
        for seed in range(3000):
            _, rows, _, _, _, _ = run_transform(config, interp, seed, sizes, 2000 + k)
            ops_applied = {r[0] for clip in rows for r in clip if not r[1]}
            skips = any(r[1] for clip in rows for r in clip)
            score = (len(ops_applied - covered), skips)
            if best is None or score > best[0]:
                best = (score, seed, ops_applied, skips)
        covered |= best[2]
        skipped |= best[3]
        chosen.append(best[1])
    assert covered == set(range(15)), ("the search did not reach every op", sorted(covered))
    assert skipped, "no case skips an op"
    for k, ((config, interp), seed) in enumerate(zip(TRANSFORM_CASES, chosen)):
        sizes = [LAND, PORT, SQUARE]
        frames, rows, mags, outs, np_after, py_after = run_transform(config, interp, seed, sizes, 2000 + k)
        case = dict(kind="transform", name=config + " " + interp, config=config, interpolation=interp, sizes=sizes,
                    data_seed=2000 + k, seed=seed, rows=rows, magnitudes=mags, np_after=repr(np_after), py_after=repr(py_after))
        case["effect_diff"] = effects(case, frames, outs)
        assert case["effect_diff"]["input"] > 0
        case["out"] = base64.b64encode(np.concatenate([o.reshape(-1) for o in outs]).tobytes()).decode()
        cases.append(case)

    import PIL
    with open(OUT, "w") as f:
        json.dump(dict(T=T, pillow=PIL.__version__, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d op, %d transform; seeds %s) -> %s, %d bytes" % (
        len(cases), sum(c["kind"] == "op" for c in cases), len(TRANSFORM_CASES), chosen, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
