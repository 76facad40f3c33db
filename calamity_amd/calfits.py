"""calfits files (pyuvdata's FITS layout for calibration solutions) <-> ``SimpleUVCal``, through the NumPy FITS subset
of ``fits.py``.  Gain-type solutions with one spectral window only.

Layout (that of pyuvdata's ``write_calfits`` for ``cal_type = "gain"``):

* primary data: float64 of NumPy shape (Nants_data, Nspws = 1, Nfreqs, Ntimes, Njones, 4), the last axis
  [gain.real, gain.imag, flag, quality].  CTYPE1..6 = Narrays, JONES, TIME, FREQS, IF, ANTAXIS; times, frequencies and
  jones are regular grids CRVAL + i CDELT (the writer refuses uneven ones).
* primary keywords: TELESCOP, ARRAYX/Y/Z, LAT/LON/ALT, GNCONVEN, CALTYPE, CALSTYLE, INTTIME, CHWIDTH, XORIENT,
  TMERANGE ("t0,t1"), HISTORY.
* ``ANTENNAS`` binary table: ANTNAME, ANTINDEX (antenna_numbers), ANTARR (ant_array, padded with -1 up to
  Nants_telescope rows), ANTXYZ (ECEF offsets from the telescope).
* ``TOTQLTY`` image: ``total_quality_array``, written when it is set.

Two additions pyuvdata ignores: the keyword ``SPWAXIS`` (T when the gain array carries the length-1 spw axis, the vintage
the reference indexes; a file without it -- a foreign one -- reads without that axis), and the image extension ``LSTS``
holding ``lst_array`` [rad], which calfits has no slot for.  A file without ``LSTS`` gets LSTs derived from the times and
the telescope longitude (``lst_from_jd``: mean sidereal time, within a few seconds of time of the apparent LST).

Antenna positions: the file holds ECEF offsets, ``SimpleUVCal.antenna_positions`` the east-north-up frame of the
``SimpleUVData`` it was built from; both directions use the rotations of ``uvh5.py`` (a synthetic object, telescope at
ECEF 0, is written at latitude = longitude = 0, where the rotation is an axis permutation and exact).
"""
import os

import numpy as np

from . import fits, uvh5

VINTAGE_KEY = "SPWAXIS"
_CTYPES = ("Narrays", "JONES", "TIME", "FREQS", "IF", "ANTAXIS")
TIME_TOL = 1e-3 / 86400.0  # [days] spacings that differ by more are uneven (pyuvdata's time tolerance, 1 ms)
FREQ_TOL = 1e-3  # [Hz] (pyuvdata's frequency tolerance)


def _regular_grid(values, tol, what, single_step):
    """(first value, step) of an evenly spaced 1-D grid; the step spans the whole grid, so every value reads back
    to within rounding."""
    values = np.asarray(values, dtype=np.float64)
    if values.size == 1:
        return float(values[0]), float(single_step)
    d = np.diff(values)
    if d.max() - d.min() > tol:
        raise ValueError(f"The {what} are not evenly spaced; the calfits format does not support unevenly spaced {what}.")
    return float(values[0]), float((values[-1] - values[0]) / (values.size - 1))


def _scalar(v, what):
    a = np.ravel(np.asarray(v, dtype=np.float64))
    if a.size == 0 or np.any(a != a[0]):
        raise ValueError(f"calfits holds one {what}; this object has {a.size} different ones")
    return float(a[0])


def _axis(hdr, n, count):
    """The values of FITS axis ``n``: CRVAL + (i + 1 - CRPIX) CDELT."""
    return float(hdr[f"CRVAL{n}"]) + (np.arange(count) + 1.0 - float(hdr.get(f"CRPIX{n}", 1))) * float(hdr[f"CDELT{n}"])


def write_calfits(uvc, path, clobber=False):
    """A gain-type ``SimpleUVCal`` (or any object with its attributes, either array vintage) -> a calfits file."""
    from .uvcompat import freqs_1d, gain4

    if os.path.exists(path) and not clobber:
        raise IOError(f"{path} exists; use clobber=True to overwrite")
    cal_type = getattr(uvc, "cal_type", "gain")
    if cal_type != "gain":
        raise ValueError(f"only gain-type calibrations are written as calfits here, not cal_type = {cal_type!r}")
    if int(getattr(uvc, "Nspws", 1)) != 1 or getattr(uvc, "flex_spw", False):
        raise ValueError("only single-spw calibrations are written as calfits here")
    spw_axis = np.ndim(uvc.gain_array) == 5
    gains, flags, quality = (gain4(np.asarray(getattr(uvc, n))) for n in ("gain_array", "flag_array", "quality_array"))
    ants = np.asarray(uvc.ant_array, dtype=np.int64)
    freqs = np.asarray(freqs_1d(uvc), dtype=np.float64)
    times = np.asarray(uvc.time_array, dtype=np.float64)
    jones = np.asarray(uvc.jones_array, dtype=np.int64)
    shape = (len(ants), len(freqs), len(times), len(jones))
    for name, a in (("gain_array", gains), ("flag_array", flags), ("quality_array", quality)):
        if a.shape != shape:
            raise ValueError(f"{name} has shape {a.shape}; ant_array, freq_array, time_array and jones_array give {shape}")
    inttime = _scalar(uvc.integration_time, "integration time")
    chwidth = _scalar(uvc.channel_width, "channel width")
    t0, dt = _regular_grid(times, TIME_TOL, "times", inttime / 86400.0)
    f0, df = _regular_grid(freqs, FREQ_TOL, "frequencies", chwidth)
    if len(jones) > 1 and len(set(np.diff(jones).tolist())) > 1:
        raise ValueError("The jones values are not evenly spaced; the calfits format does not support unevenly spaced jones values.")
    dj = int(jones[1] - jones[0]) if len(jones) > 1 else -1

    loc = np.asarray(getattr(uvc, "telescope_location", np.zeros(3)), dtype=np.float64)
    lat, lon, alt = uvh5.lat_lon_alt_from_ecef(loc)
    cards = [
        ("TELESCOP", str(uvc.telescope_name)), ("GNCONVEN", str(uvc.gain_convention)), ("CALTYPE", cal_type),
        ("CALSTYLE", str(getattr(uvc, "cal_style", "redundant"))), ("INTTIME", inttime), ("CHWIDTH", chwidth),
        ("XORIENT", getattr(uvc, "x_orientation", None)),
    ]
    if getattr(uvc, "time_range", None) is not None:
        cards.append(("TMERANGE", ",".join(repr(float(t)) for t in uvc.time_range)))
    axes = (
        ("Integer", 1, 1, "Number of image arrays."),
        ("Integer", int(jones[0]), dj, "Jones matrix array"),
        ("JD", t0, dt, "Time axis."),
        ("Hz", f0, df, "Frequency."),
        ("Integer", 1, 1, "Spectral window number."),
        ("Integer", 0, -1, "See ANTARR in ANTENNA extension for values."),
    )
    for n, (ctype, (unit, crval, cdelt, comment)) in enumerate(zip(_CTYPES, axes), start=1):
        cards += [(f"CTYPE{n}", ctype, comment), (f"CUNIT{n}", unit), (f"CRPIX{n}", 1), (f"CRVAL{n}", crval), (f"CDELT{n}", cdelt)]
    cards += [(VINTAGE_KEY, spw_axis, "gain array with a length-1 spw axis"),
              ("ARRAYX", float(loc[0])), ("ARRAYY", float(loc[1])), ("ARRAYZ", float(loc[2])),
              ("LAT", lat), ("LON", lon), ("ALT", alt)]
    cards += [("HISTORY", line) for line in str(getattr(uvc, "history", "") or "").splitlines()]

    data = np.empty((shape[0], 1) + shape[1:] + (4,), dtype=np.float64)
    data[:, 0, ..., 0] = gains.real
    data[:, 0, ..., 1] = gains.imag
    data[:, 0, ..., 2] = flags
    data[:, 0, ..., 3] = quality
    hdus = [fits.image_hdu(data, cards, primary=True)]

    names = [str(s) for s in uvc.antenna_names]
    nants_tel = len(names)
    if len(ants) > nants_tel:
        raise ValueError(f"ant_array holds {len(ants)} antennas, the telescope {nants_tel}")
    enu = np.asarray(uvc.antenna_positions, dtype=np.float64)
    hdus.append(fits.bintable_hdu([
        ("ANTNAME", f"{max([8] + [len(s) for s in names])}A", names),
        ("ANTINDEX", "D", np.asarray(uvc.antenna_numbers, dtype=np.float64)),
        ("ANTARR", "D", np.concatenate([ants, -np.ones(nants_tel - len(ants), dtype=np.int64)]).astype(np.float64)),
        ("ANTXYZ", "3D", uvh5.ecef_offsets_from_enu(enu, lat, lon)),
    ], name="ANTENNAS"))
    tot = getattr(uvc, "total_quality_array", None)
    if tot is not None:
        tot = np.asarray(tot, dtype=np.float64)
        tot = tot if tot.ndim == 4 else tot[None]  # (Nspws, Nfreqs, Ntimes, Njones) in the file
        tcards = []
        for n, (ctype, (unit, crval, cdelt, comment)) in enumerate(zip(_CTYPES[1:5], axes[1:5]), start=1):
            tcards += [(f"CTYPE{n}", ctype, comment), (f"CUNIT{n}", unit), (f"CRPIX{n}", 1), (f"CRVAL{n}", crval), (f"CDELT{n}", cdelt)]
        hdus.append(fits.image_hdu(tot, tcards, name="TOTQLTY"))
    lsts = getattr(uvc, "lst_array", None)
    if lsts is not None and np.size(lsts) == len(times):
        hdus.append(fits.image_hdu(np.asarray(lsts, dtype=np.float64).reshape(-1), name="LSTS"))
    fits.write(path, hdus)


def lst_from_jd(jd, lon_deg):
    """Local mean sidereal time [rad] at Julian dates ``jd`` (UT1 taken as UTC) and east longitude ``lon_deg``: the IAU
    2006 Earth rotation angle plus its GMST polynomial.  It differs from the apparent LST pyuvdata computes by the
    equation of the equinoxes and UT1 - UTC, a few seconds of time at most."""
    jd = np.asarray(jd, dtype=np.float64)
    du = jd - 2451545.0
    era = 2.0 * np.pi * ((0.7790572732640 + 0.00273781191135448 * du + du) % 1.0)
    t = du / 36525.0
    arcsec = 0.014506 + 4612.156534 * t + 1.3915817 * t ** 2 - 0.00000044 * t ** 3 - 0.000029956 * t ** 4
    return (era + np.radians(arcsec / 3600.0) + np.radians(lon_deg)) % (2.0 * np.pi)


def _read_one(path):
    from .uvcompat import SimpleUVCal

    with fits.open(path) as f:
        hdr = f[0].header
        if hdr.get("CALTYPE") != "gain":
            raise ValueError(f"{path}: CALTYPE = {hdr.get('CALTYPE')!r}; only gain-type calfits files are supported")
        got = tuple(str(hdr.get(f"CTYPE{n}", "")).strip() for n in range(1, 7))
        if got != _CTYPES or f[0].header.get("NAXIS") != 6:
            raise ValueError(f"{path}: primary axes {got}; a gain calfits file has {_CTYPES}")
        if "ANTENNAS" not in f:
            raise ValueError(f"{path}: no ANTENNAS extension")
        data = f[0].data
        ant = f["ANTENNAS"].data
        tot = f["TOTQLTY"].data if "TOTQLTY" in f else None
        lsts = f["LSTS"].data if "LSTS" in f else None
    nants, nspws, nfreqs, ntimes, njones, narrays = data.shape
    if nspws != 1:
        raise ValueError(f"{path}: {nspws} spectral windows; only single-spw calfits files are supported")
    if narrays != 4:
        raise ValueError(f"{path}: {narrays} arrays per sample; a gain calfits file has 4 (real, imag, flag, quality)")
    spw_axis = bool(hdr.get(VINTAGE_KEY, False))

    uvc = SimpleUVCal()
    uvc.cal_type = "gain"
    uvc.cal_style = hdr.get("CALSTYLE")
    uvc.gain_convention = hdr.get("GNCONVEN")
    uvc.telescope_name = hdr.get("TELESCOP")
    uvc.x_orientation = hdr.get("XORIENT")
    uvc.history = "\n".join(hdr.commentary("HISTORY"))
    if "ARRAYX" in hdr:
        uvc.telescope_location = np.array([float(hdr[k]) for k in ("ARRAYX", "ARRAYY", "ARRAYZ")])
    else:
        uvc.telescope_location = uvh5.ecef_from_lat_lon_alt(float(hdr["LAT"]), float(hdr["LON"]), float(hdr["ALT"]))
    if "LAT" in hdr and "LON" in hdr:
        lat, lon = float(hdr["LAT"]), float(hdr["LON"])
    else:
        lat, lon, _ = uvh5.lat_lon_alt_from_ecef(uvc.telescope_location)
    uvc.antenna_names = [str(s) for s in ant["ANTNAME"]]
    uvc.antenna_numbers = np.rint(ant["ANTINDEX"]).astype(np.int64)
    uvc.antenna_positions = uvh5.enu_from_ecef_offsets(ant["ANTXYZ"], lat, lon)
    uvc.Nants_telescope = len(uvc.antenna_names)
    antarr = np.rint(ant["ANTARR"]).astype(np.int64)
    uvc.ant_array = antarr[antarr >= 0]
    if len(uvc.ant_array) != nants:
        raise ValueError(f"{path}: ANTARR names {len(uvc.ant_array)} antennas, the data hold {nants}")
    uvc.Nfreqs, uvc.Ntimes, uvc.Njones, uvc.Nspws = nfreqs, ntimes, njones, 1
    uvc.spw_array = np.array([0])
    freqs = _axis(hdr, 4, nfreqs)
    uvc.freq_array = freqs[None, :] if spw_axis else freqs
    uvc.channel_width = np.float64(hdr["CHWIDTH"])
    uvc.time_array = _axis(hdr, 3, ntimes)
    uvc.integration_time = np.float64(hdr["INTTIME"])
    uvc.jones_array = np.rint(_axis(hdr, 2, njones)).astype(np.int64)
    tr = hdr.get("TMERANGE")
    uvc.time_range = tuple(float(t) for t in tr.split(",")) if tr else None
    uvc.lst_array = lsts.astype(np.float64) if lsts is not None and lsts.shape == (ntimes,) else lst_from_jd(uvc.time_array, lon)

    sl = (slice(None), slice(None)) if spw_axis else (slice(None), 0)
    uvc.gain_array = np.empty(data[sl + (Ellipsis, 0)].shape, dtype=np.complex128)
    uvc.gain_array.real = data[sl + (Ellipsis, 0)]
    uvc.gain_array.imag = data[sl + (Ellipsis, 1)]
    uvc.flag_array = data[sl + (Ellipsis, 2)] != 0.0
    uvc.quality_array = np.ascontiguousarray(data[sl + (Ellipsis, 3)])
    if tot is not None:
        if tot.shape != (1, nfreqs, ntimes, njones):
            raise ValueError(f"{path}: TOTQLTY has shape {tot.shape}, expected {(1, nfreqs, ntimes, njones)}")
        tot = tot if spw_axis else tot[0]
    uvc.total_quality_array = tot
    return uvc


def concat_times(objs, names):
    """Gain objects of the same antennas, frequencies and jones at different times -> one object (time-ordered),
    through ``SimpleUVCal.__add__``; ``lst_array``, ``time_range`` and ``total_quality_array`` follow."""
    from .uvcompat import freqs_1d

    out = objs[0]
    for obj, name in zip(objs[1:], names[1:]):
        if np.ndim(obj.gain_array) != np.ndim(out.gain_array):
            raise ValueError(f"{name}: its gain array is of another vintage (with / without the spw axis) than {names[0]}'s")
        for attr, a, b in (("antennas", out.ant_array, obj.ant_array), ("frequencies", freqs_1d(out), freqs_1d(obj)),
                           ("jones values", out.jones_array, obj.jones_array)):
            if not np.array_equal(np.asarray(a), np.asarray(b)):
                raise ValueError(f"{name}: its {attr} differ from those of {names[0]}")
        t1, t2 = np.asarray(out.time_array), np.asarray(obj.time_array)
        if np.any(np.isclose(t1[:, None], t2[None, :], rtol=0.0, atol=1e-7)):
            raise ValueError(f"{name} holds a time that an earlier gain file already holds")
        order = np.argsort(np.concatenate([t1, t2]))  # (the order __add__ sorts into)
        lsts = [getattr(o, "lst_array", None) for o in (out, obj)]
        tots = [getattr(o, "total_quality_array", None) for o in (out, obj)]
        ranges = [getattr(o, "time_range", None) for o in (out, obj)]
        out = out + obj
        out.lst_array = np.concatenate(lsts)[order] if all(x is not None for x in lsts) else None
        out.total_quality_array = (np.take(np.concatenate(tots, axis=-2), order, axis=-2)
                                   if all(x is not None for x in tots) else None)
        if all(r is not None for r in ranges):
            out.time_range = (min(ranges[0][0], ranges[1][0]), max(ranges[0][1], ranges[1][1]))
    return out


def read_calfits(path):
    """A calfits file, or a list of them concatenated along time, -> ``SimpleUVCal``."""
    if isinstance(path, (list, tuple)):
        return concat_times([_read_one(p) for p in path], [str(p) for p in path])
    return _read_one(path)
