"""Time writing and re-reading a uvh5 file at a BASELINE size (one time of HERA-350: 61 425 baselines with the autos,
1024 channels, one polarization) with calamity_amd's own uvh5 writer and reader, next to np.fromfile of the same bytes.

    python tools/uvh5_io_bench.py [--dir DIR] [--nants 350] [--nfreqs 1024]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from calamity_amd import hdf5, uvh5  # noqa: E402
from calamity_amd.uvcompat import SimpleUVData  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where to write the file (default: the system's temporary directory)")
    ap.add_argument("--nants", type=int, default=350)
    ap.add_argument("--nfreqs", type=int, default=1024)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(args.nants)))
    pos = np.asarray([[14.6 * (k % side), 14.6 * (k // side), 0.0] for k in range(args.nants)])
    pairs = [(i, j) for i in range(args.nants) for j in range(i, args.nants)]
    uvd = SimpleUVData(pos, pairs, np.linspace(100e6, 200e6, args.nfreqs), [2459000.5], x_orientation="east")
    uvd.data_array = (rng.standard_normal(uvd.data_array.shape) + 1j * rng.standard_normal(uvd.data_array.shape))
    gib = uvd.data_array.nbytes / 2 ** 30
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "hera.uvh5")
        t0 = time.perf_counter()
        uvd.write_uvh5(path)
        t_write = time.perf_counter() - t0
        size = os.path.getsize(path) / 2 ** 30
        t0 = time.perf_counter()
        back = uvh5.read_uvh5(path)
        t_read = time.perf_counter() - t0
        assert np.array_equal(back.data_array, uvd.data_array)
        t0 = time.perf_counter()
        with hdf5.open(path) as f:  # (opening is part of the time: it parses the metadata)
            vis = f["Data/visdata"][()]
            addr = f["Data/visdata"]._layout[1]
        t_vis = time.perf_counter() - t0
        t0 = time.perf_counter()
        raw = np.fromfile(path, dtype=np.complex128, count=vis.size, offset=addr)
        t_fromfile = time.perf_counter() - t0
        assert np.array_equal(raw, vis.ravel())
    print(f"{uvd.Nblts} rows x {uvd.Nfreqs} channels x {uvd.Npols} pol: visibilities {gib:.2f} GiB, file {size:.2f} GiB")
    print(f"write_uvh5 {t_write:.2f} s, read_uvh5 {t_read:.2f} s (hdf5.open + Data/visdata {t_vis:.2f} s; np.fromfile of the same "
          f"bytes {t_fromfile:.2f} s)")


if __name__ == "__main__":
    main()
