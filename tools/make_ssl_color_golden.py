"""Records tests/golden/ssl_color_contract.json: the SSL colour stage (``transform.color_jitter_video_ssl``) restated with PIL on
the CPU.  Needs Pillow; neither torchvision nor the reference tree.

    python tools/make_ssl_color_golden.py

torchvision's PIL backend is a handful of PIL calls, and those very calls are made here on the (T * h) x w stack of a clip's
frames, which is the one image the reference hands to torchvision:

* brightness, contrast, saturation: ``ImageEnhance.Brightness / Contrast / Color(img).enhance(factor)``;
* hue: ``img.convert("HSV")``, ``H += uint8(hue_factor * 255)`` with wrap-around, ``Image.merge("HSV", ...).convert("RGB")``;
* RandomGrayscale: ``img.convert("L")`` replicated to three channels;
* GaussianBlur: ``img.filter(ImageFilter.GaussianBlur(radius=sigma))``.

The DRAW is ``slowfast_amd.SslColorJitter.sample_batch`` under ``torch.manual_seed(seed)`` / ``random.seed(seed)``: torchvision is
not available to draw it, so the fixture pins this package's restatement of its published behaviour against later changes, not
against torchvision (tests/ssl_color_checks.py:restate_draw states it a second time).  Per case the file holds the parameters,
the seed, the rows, one more draw from each generator (where they stand afterwards) and PIL's output bytes for the frames
tests/ssl_color_checks.py:case_frames draws again.  The numpy restatement in that module must reproduce every byte.
"""
import base64
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ssl_color_contract.json")
sys.path.insert(0, ROOT)

MOCO = dict(bri_con_sat=[0.6, 0.6, 0.6], hue=0.15, p_convert_gray=0.2, moco_v2_aug=True)      # configs/contrastive_ssl/*
PLAIN = dict(bri_con_sat=[0.4, 0.4, 0.4], hue=0.1, p_convert_gray=0.2, moco_v2_aug=False)
# (name, parameters, seed)
CASES = [("MoCo-v2 branch, seed 0", MOCO, 0), ("MoCo-v2 branch, seed 5", MOCO, 5), ("MoCo-v2 branch, seed 11", MOCO, 11),
         ("MoCo-v2 branch, always grey", dict(MOCO, p_convert_gray=1.0), 3),
         ("plain branch, seed 0", PLAIN, 0), ("plain branch, seed 1", PLAIN, 1),
         ("plain branch, always grey, no contrast jitter", dict(PLAIN, bri_con_sat=[0.4, 0.0, 0.4], p_convert_gray=1.0), 4)]


def pil_clip(frames, row, gray_first):
    """One clip, uint8 (T, h, w, 3), through PIL as torchvision's PIL backend drives it."""
    from PIL import Image, ImageEnhance, ImageFilter
    img = Image.fromarray(np.ascontiguousarray(frames.reshape(-1, frames.shape[2], 3)), "RGB")

    def gray(im):
        return Image.fromarray(np.stack([np.array(im.convert("L"))] * 3, axis=-1), "RGB")

    def hue(im, factor):
        h, s, v = im.convert("HSV").split()
        np_h = ((np.array(h, dtype=np.uint8).astype(np.int64) + int(factor * 255)) % 256).astype(np.uint8)
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    if gray_first and row.gray:
        img = gray(img)
    if row.jitter:
        for op in row.order:
            if op == 0 and row.brightness is not None:
                img = ImageEnhance.Brightness(img).enhance(row.brightness)
            elif op == 1 and row.contrast is not None:
                img = ImageEnhance.Contrast(img).enhance(row.contrast)
            elif op == 2 and row.saturation is not None:
                img = ImageEnhance.Color(img).enhance(row.saturation)
            elif op == 3 and row.hue is not None:
                img = hue(img, row.hue)
    if not gray_first and row.gray:
        img = gray(img)
    if row.sigma is not None:
        img = img.filter(ImageFilter.GaussianBlur(radius=row.sigma))
    return np.asarray(img).reshape(frames.shape)


def main():
    import PIL
    import torch
    import slowfast_amd as sa
    from tests import ssl_color_checks as checks
    T = 3
    checks.T = T
    cases = []
    for k, (name, params, seed) in enumerate(CASES):
        fn = sa.SslColorJitter(**params)
        torch.manual_seed(seed)
        random.seed(seed)
        table = fn.sample_batch(len(checks.SIZES))
        torch_after, py_after = checks.positions()
        frames = checks.case_frames(50 + k)
        out = [pil_clip(f.numpy(), table.rows[n], table.gray_first) for n, f in enumerate(frames)]
        restated = checks.restate_batch(frames, table)
        for n in range(len(frames)):
            diff = checks.differing(restated[n], out[n])
            assert diff == 0, "%s, sample %d: the numpy restatement differs from PIL in %d bytes" % (name, n, diff)
        print("%-50s %s" % (name, ["%s%s%s" % ("J" if r.jitter else "-", "G" if r.gray else "-", "B" if r.sigma is not None else "-")
                                    for r in table.rows]))
        cases.append(dict(name=name, seed=seed, data_seed=50 + k, sizes=[list(s) for s in checks.SIZES], gray_first=table.gray_first,
                          rows=[checks.row_to_json(r) for r in table.rows], torch_after=torch_after, py_after=py_after,
                          out=base64.b64encode(b"".join(np.ascontiguousarray(o).tobytes() for o in out)).decode(), **params))
    with open(OUT, "w") as f:
        json.dump(dict(T=T, pillow=PIL.__version__, torch=torch.__version__.split("+")[0], cases=cases), f, indent=1)
        f.write("\n")
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
