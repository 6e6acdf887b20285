#!/usr/bin/env python
"""Record tests/golden/imresize_ref.npz: the reference's float32 `imresize` (basicsr/utils/matlab_functions.py, loaded by path: it needs
only torch and numpy) on seeded [0,1] inputs.

    python tests/golden/make_golden_imresize.py /path/to/reference [out.npz]

Inputs 5x7, 9x11, 24x37 and 48x48; scales 0.5, 0.25, 1/3, 0.7, 1.5, 2 and 4; both antialiasing settings.  Only the cases the reference
completes are recorded (it raises where its symmetric padding is longer than the image, e.g. 24x37 at 0.25 without antialiasing).
Keys: in_<H>x<W> (float32 input), cases (one 'HxW|scale index|aa' string per recorded case), out_<case index> (float32 output);
scales (float64, the exact values passed).
"""
import importlib.util
import os
import sys

import numpy as np

SIZES = ((5, 7), (9, 11), (24, 37), (48, 48))
SCALES = (0.5, 0.25, 1 / 3, 0.7, 1.5, 2, 4)


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'imresize_ref.npz')
    spec = importlib.util.spec_from_file_location('matlab_functions', os.path.join(ref, 'basicsr', 'utils', 'matlab_functions.py'))
    mf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mf)
    import torch
    rng = np.random.RandomState(20240)
    data, cases = {'scales': np.array(SCALES, dtype=np.float64)}, []
    for h, w in SIZES:
        x = rng.rand(h, w).astype(np.float32)
        data[f'in_{h}x{w}'] = x
        for si, scale in enumerate(SCALES):
            for aa in (True, False):
                try:
                    y = mf.imresize(torch.from_numpy(x.copy()), scale, antialiasing=aa).numpy()
                except Exception as e:          # the reference does not complete this case
                    print(f'{h}x{w} scale {scale:.4g} aa={aa}: reference raises {type(e).__name__}')
                    continue
                if not np.isfinite(y).all():
                    print(f'{h}x{w} scale {scale:.4g} aa={aa}: non-finite output, not recorded')
                    continue
                data[f'out_{len(cases)}'] = y.astype(np.float32)
                cases.append(f'{h}x{w}|{si}|{int(aa)}')
    data['cases'] = np.array(cases)
    np.savez_compressed(out, **data)
    print(f'{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)')


if __name__ == '__main__':
    main()
