"""Writes foreign_gain.calfits: a gain calfits file in the layout of pyuvdata's UVCal.write_calfits (cal_type "gain",
one spectral window), written with astropy.io.fits -- a FITS implementation independent of calamity_amd/fits.py.
tests/test_calfits.py reads it with the package's own reader and checks every value against the constants and
formulas below (it imports this file; only main() needs astropy).

Run with an interpreter that has astropy (checked with astropy 4.3.1):  python make_calfits.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

ANTENNA_NUMBERS = [9, 10, 20, 53]
ANTENNA_NAMES = ["HH9", "HH10", "HH20", "HH53"]
ANT_ARRAY = [10, 20, 53]  # Nants_data = 3 < Nants_telescope = 4
NFREQS, NTIMES, NJONES = 8, 3, 2
FREQ0, DFREQ = 100e6, 97656.25
INTTIME = 10.737418240000001
TIME0 = 2459122.25
JONES0 = -5
ARRAY_XYZ = (5109342.76037543, 2005241.90402741, -3239939.46926407)
LAT, LON, ALT = -30.721526120689507, 21.428303826863015, 1051.6900000218302
TIME_RANGE = (TIME0 - 0.5 * INTTIME / 86400.0, TIME0 + (NTIMES - 0.5) * INTTIME / 86400.0)
HISTORY = ["Written by make_calfits.py in the layout of pyuvdata's write_calfits. " + "h" * 30, "second line"]


def arrays():
    """gain, flag, quality (NumPy axes Nants_data, Nfreqs, Ntimes, Njones) and total quality (Nfreqs, Ntimes, Njones):
    dyadic rationals, exact in float64."""
    a, f, t, j = np.meshgrid(np.arange(len(ANT_ARRAY)), np.arange(NFREQS), np.arange(NTIMES), np.arange(NJONES), indexing="ij")
    gain = (1.0 + (a * 64 + f * 8 + t * 2 + j) / 1024.0) + 1j * (((a + 1) * (f + 1) - t - 3 * j) / 512.0)
    flag = (a + f + t + j) % 5 == 0
    quality = (a * f + t * j) / 16.0
    f3, t3, j3 = np.meshgrid(np.arange(NFREQS), np.arange(NTIMES), np.arange(NJONES), indexing="ij")
    total = (f3 + 10 * t3 + 100 * j3) / 8.0
    return gain, flag, quality, total


def antenna_xyz():
    """ECEF offsets [m] of the telescope's antennas."""
    n = np.arange(len(ANTENNA_NUMBERS), dtype=np.float64)
    return np.stack([n * 14.5 - 3.25, -n * 6.0 + 0.5, n * n * 0.75], axis=-1)


def main():
    # astropy 4.3 predates NumPy 1.26, which dropped these two
    np.asscalar = lambda a: a.item()
    np.alen = len
    from astropy.io import fits

    gain, flag, quality, total = arrays()
    hdr = fits.Header()
    hdr["TELESCOP"] = "HERA"
    hdr["GNCONVEN"] = "divide"
    hdr["CALTYPE"] = "gain"
    hdr["CALSTYLE"] = "redundant"
    hdr["INTTIME"] = INTTIME
    hdr["CHWIDTH"] = DFREQ
    hdr["XORIENT"] = "east"
    hdr["TMERANGE"] = ",".join(map(str, TIME_RANGE))
    axes = [("Narrays", "Integer", 1, 1), ("JONES", "Integer", JONES0, -1), ("TIME", "JD", TIME0, INTTIME / 86400.0),
            ("FREQS", "Hz", FREQ0, DFREQ), ("IF", "Integer", 1, 1), ("ANTAXIS", "Integer", 0, -1)]
    for n, (ctype, cunit, crval, cdelt) in enumerate(axes, start=1):
        hdr[f"CTYPE{n}"] = ctype
        hdr[f"CUNIT{n}"] = cunit
        hdr[f"CRPIX{n}"] = 1
        hdr[f"CRVAL{n}"] = crval
        hdr[f"CDELT{n}"] = cdelt
    for k, v in zip(("ARRAYX", "ARRAYY", "ARRAYZ", "LAT", "LON", "ALT"), ARRAY_XYZ + (LAT, LON, ALT)):
        hdr[k] = v
    for line in HISTORY:
        hdr.add_history(line)
    data = np.stack([gain.real, gain.imag, flag.astype(np.float64), quality], axis=-1)[:, None]
    primary = fits.PrimaryHDU(data=data, header=hdr)

    cols = fits.ColDefs([
        fits.Column(name="ANTNAME", format="8A", array=np.asarray(ANTENNA_NAMES)),
        fits.Column(name="ANTINDEX", format="D", array=np.asarray(ANTENNA_NUMBERS, dtype=np.float64)),
        fits.Column(name="ANTARR", format="D", array=np.asarray(ANT_ARRAY + [-1], dtype=np.float64)),
        fits.Column(name="ANTXYZ", format="3D", array=antenna_xyz()),
    ])
    ants = fits.BinTableHDU.from_columns(cols)
    ants.header["EXTNAME"] = "ANTENNAS"
    tot = fits.ImageHDU(data=total[None])
    tot.header["EXTNAME"] = "TOTQLTY"
    hdul = fits.HDUList([primary, ants, tot])
    hdul.verify("exception")
    out = os.path.join(HERE, "foreign_gain.calfits")
    hdul.writeto(out, overwrite=True)
    with fits.open(out) as f:
        f.verify("exception")


if __name__ == "__main__":
    main()
