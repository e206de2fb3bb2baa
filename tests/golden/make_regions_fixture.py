"""Writes tests/golden/regions/data_regions.npz: detector-region image features for the dialogs of the committed prepro fixture
(tests/golden/prepro/), in the form `-imgRegions 9 -inputImg .../data_regions.npz` reads (visdial_amd/dataloader.py _open_arrays):

    regions_<split>      float32 [n x M x C]   M = 9 region rows of C = 8 channels, non-negative like pooled detector features; the rows
                                               behind an image's count hold 1e3 on purpose: the loader has to zero them
    num_regions_<split>  int32   [n]           live regions of every image, 1 .. M; every split holds a 1 and a 9

n = the number of images of the split in the prepro fixture (img_pos_<split> of visdial_data.h5 indexes them).  Fixed seed:
    python tests/golden/make_regions_fixture.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
M, C, SEED = 9, 8, 20240917


def main():
    pre = np.load(os.path.join(HERE, 'prepro', 'expected.npz'))
    rng = np.random.RandomState(SEED)
    out = {}
    for split in ('train', 'val', 'test'):
        n = int(pre['img.images_' + split].shape[0])
        assert n >= 2 and int(pre['data.img_pos_' + split].max()) < n
        cnt = rng.randint(1, M + 1, size=n).astype(np.int32)
        cnt[0], cnt[n - 1] = 1, M
        f = np.abs(rng.randn(n, M, C)).astype(np.float32)
        f[np.arange(M)[None, :] >= cnt[:, None]] = 1e3
        out['regions_' + split], out['num_regions_' + split] = f, cnt
    os.makedirs(os.path.join(HERE, 'regions'), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, 'regions', 'data_regions.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
