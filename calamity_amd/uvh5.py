"""uvh5 files (pyuvdata's HDF5 layout) <-> ``SimpleUVData``, through the NumPy HDF5 subset of ``hdf5.py``.

A file holds two groups: ``Header`` (the metadata, one dataset per UVData attribute) and ``Data`` (``visdata``, a
compound {r, i}; ``flags``, an 8-bit enum; ``nsamples``).  Visibilities carry the spw axis when ``visdata`` is 4-D and
use pyuvdata's "future array shapes" when it is 3-D.  One spectral window only.

Antenna positions: the file stores ECEF offsets from the telescope, ``SimpleUVData.antenna_positions`` holds the local
east-north-up frame (the one the fit uses).  The rotation between them never moves an exact zero: an object read from
a file writes its original ECEF array back when its ENU positions are unchanged, and a synthetic object (telescope
location 0) is written at latitude = longitude = 0, where the rotation is an axis permutation.
"""
import os

import numpy as np

from . import hdf5

# WGS84
_A = 6378137.0
_F = 1.0 / 298.257223563
_E2 = _F * (2.0 - _F)

_STRINGS = ("history", "instrument", "object_name", "phase_type", "vis_units", "version")
_STRING_DEFAULTS = {"history": "", "instrument": None, "object_name": "zenith", "phase_type": "drift", "vis_units": "uncalib",
                    "version": "1.0"}
# the Header datasets a synthetic object is written with (x_orientation added when set)
_STANDARD = ("Nants_data", "Nants_telescope", "Nbls", "Nblts", "Nfreqs", "Npols", "Nspws", "Ntimes", "altitude", "ant_1_array",
             "ant_2_array", "antenna_names", "antenna_numbers", "antenna_positions", "channel_width", "freq_array", "history",
             "instrument", "integration_time", "latitude", "longitude", "lst_array", "object_name", "phase_type",
             "polarization_array", "spw_array", "telescope_name", "time_array", "uvw_array", "version", "vis_units")


def _rotation(lat_deg, lon_deg):
    """Rows: the east, north and up unit vectors in ECEF at (lat, lon)."""
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    sp, cp, sl, cl = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return np.array([[-sl, cl, 0.0], [-sp * cl, -sp * sl, cp], [cp * cl, cp * sl, sp]])


def enu_from_ecef_offsets(xyz, lat_deg, lon_deg):
    """ECEF offsets from the telescope [m] -> east, north, up [m] (component by component, no matrix product)."""
    r = _rotation(lat_deg, lon_deg)
    xyz = np.asarray(xyz, dtype=np.float64)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return np.stack([r[k, 0] * x + r[k, 1] * y + r[k, 2] * z for k in range(3)], axis=-1)


def ecef_offsets_from_enu(enu, lat_deg, lon_deg):
    r = _rotation(lat_deg, lon_deg)
    enu = np.asarray(enu, dtype=np.float64)
    e, n, u = enu[..., 0], enu[..., 1], enu[..., 2]
    return np.stack([r[0, k] * e + r[1, k] * n + r[2, k] * u for k in range(3)], axis=-1)


def ecef_from_lat_lon_alt(lat_deg, lon_deg, alt):
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    n = _A / np.sqrt(1.0 - _E2 * np.sin(lat) ** 2)
    return np.array([(n + alt) * np.cos(lat) * np.cos(lon), (n + alt) * np.cos(lat) * np.sin(lon), (n * (1.0 - _E2) + alt) * np.sin(lat)])


def lat_lon_alt_from_ecef(xyz):
    x, y, z = (float(v) for v in xyz)
    if x == 0.0 and y == 0.0 and z == 0.0:
        return 0.0, 0.0, 0.0
    lon = np.arctan2(y, x)
    p = np.hypot(x, y)
    lat = np.arctan2(z, p * (1.0 - _E2))
    for _ in range(10):
        n = _A / np.sqrt(1.0 - _E2 * np.sin(lat) ** 2)
        alt = p / np.cos(lat) - n
        lat = np.arctan2(z, p * (1.0 - _E2 * n / (n + alt)))
    n = _A / np.sqrt(1.0 - _E2 * np.sin(lat) ** 2)
    return float(np.degrees(lat)), float(np.degrees(lon)), float(p / np.cos(lat) - n)


# per-row (Nblts) Header datasets of newer pyuvdata files that this module does not derive: sliced by ``select``,
# concatenated by ``__add__`` (uvcompat.py), so a written file stays consistent
PER_BLT = ("phase_center_id_array", "phase_center_app_ra", "phase_center_app_dec", "phase_center_frame_pa")


def header_rows(hdr, keep):
    """The Header dict of an object whose rows were selected with the boolean mask ``keep``."""
    out = dict(hdr)
    for k in PER_BLT:
        if k in out:
            out[k] = np.asarray(out[k])[keep]
    return out


def header_concat(h1, h2):
    """The Header dict of the row concatenation of two objects (per-row fields the second one lacks are dropped)."""
    out = dict(h1)
    for k in PER_BLT:
        if k in out:
            if h2 and k in h2:
                out[k] = np.concatenate([np.asarray(out[k]), np.asarray(h2[k])])
            else:
                del out[k]
    return out


def _read_tree(group):
    """A group's members: datasets as arrays, subgroups (pyuvdata's ``extra_keywords``, ``phase_center_catalog``) as
    nested dicts, which ``hdf5.write`` turns back into groups."""
    out = {}
    for k in group.keys():
        v = group[k]
        out[k] = _read_tree(v) if isinstance(v, hdf5.Group) else v[()]
    return out


def _str(v):
    return bytes(np.asarray(v).item()).decode("utf-8")


def read_uvh5(path):
    """A uvh5 file -> ``SimpleUVData`` (all rows, all channels, all polarizations)."""
    from .uvcompat import SimpleUVData

    with hdf5.open(path) as f:
        if "Header" not in f or "Data/visdata" not in f:
            raise ValueError(f"{path}: not a uvh5 file (no Header group or Data/visdata)")
        hdr = _read_tree(f["Header"])
        if int(hdr.get("Nspws", 1)) > 1:
            raise ValueError(f"{path}: {int(hdr['Nspws'])} spectral windows; only single-spw uvh5 files are supported")
        if "flex_spw" in hdr and bool(hdr["flex_spw"]):
            raise ValueError(f"{path}: flex_spw files are not supported")
        vis = f["Data/visdata"][()]
        flags = f["Data/flags"][()]
        nsamples = f["Data/nsamples"][()]
    if vis.ndim not in (3, 4) or flags.shape != vis.shape or nsamples.shape != vis.shape:
        raise ValueError(f"{path}: Data/visdata, flags and nsamples must share a 3-D or 4-D shape")
    future = vis.ndim == 3

    uvd = object.__new__(SimpleUVData)
    uvd.uvh5_header = hdr  # every Header dataset as stored: write_uvh5 reproduces the ones it does not derive
    lat, lon, alt = (float(hdr[k]) for k in ("latitude", "longitude", "altitude"))
    uvd.telescope_location = ecef_from_lat_lon_alt(lat, lon, alt)
    uvd.telescope_name = _str(hdr["telescope_name"])
    for name in _STRINGS:
        if name in hdr:
            setattr(uvd, name, _str(hdr[name]))
    uvd.antenna_numbers = np.asarray(hdr["antenna_numbers"])
    uvd.antenna_names = [_str(n) for n in np.atleast_1d(hdr["antenna_names"])]
    uvd.antenna_positions = enu_from_ecef_offsets(hdr["antenna_positions"], lat, lon)
    uvd.Nants_telescope = int(hdr["Nants_telescope"])
    for name in ("ant_1_array", "ant_2_array", "time_array", "lst_array", "integration_time", "uvw_array"):
        setattr(uvd, name, np.asarray(hdr[name]))
    uvd.future_array_shapes = future
    freqs = np.asarray(hdr["freq_array"], dtype=np.float64).reshape(-1)
    uvd.freq_array = freqs if future else freqs[None, :]
    uvd.Nfreqs = freqs.size
    uvd.Nspws = 1
    uvd.spw_array = np.asarray(hdr["spw_array"])
    cw = np.asarray(hdr["channel_width"])
    uvd.channel_width = float(cw) if cw.ndim == 0 else cw
    uvd.polarization_array = np.asarray(hdr["polarization_array"])
    uvd.Npols = uvd.polarization_array.size
    uvd.x_orientation = _str(hdr["x_orientation"]) if "x_orientation" in hdr else None
    uvd.data_array = vis  # complex128 or complex64, as stored (written back in the same precision)
    uvd.flag_array = flags
    uvd.nsample_array = nsamples.astype(np.float64)
    uvd._refresh()
    if uvd.Nfreqs != vis.shape[-2] or uvd.Npols != vis.shape[-1] or uvd.Nblts != vis.shape[0]:
        raise ValueError(f"{path}: Data/visdata shape {vis.shape} does not match the header")
    return uvd


def _uvw(uvd):
    pos = {int(a): p for a, p in zip(uvd.antenna_numbers, np.asarray(uvd.antenna_positions, dtype=np.float64))}
    a1 = np.asarray(uvd.ant_1_array).tolist()
    a2 = np.asarray(uvd.ant_2_array).tolist()
    return np.asarray([pos[b] - pos[a] for a, b in zip(a1, a2)], dtype=np.float64).reshape(-1, 3)


def write_uvh5(uvd, path, clobber=False):
    """``SimpleUVData`` (or any object with its attributes) -> a uvh5 file with the datasets and types pyuvdata writes.
    An object read by ``read_uvh5`` writes back every Header dataset the file had."""
    if os.path.exists(path) and not clobber:
        raise IOError(f"{path} exists; use clobber=True to overwrite")
    raw = dict(getattr(uvd, "uvh5_header", None) or {})
    if raw:
        lat, lon, alt = (float(raw[k]) for k in ("latitude", "longitude", "altitude"))
    else:
        lat, lon, alt = lat_lon_alt_from_ecef(getattr(uvd, "telescope_location", np.zeros(3)))
    enu = np.asarray(uvd.antenna_positions, dtype=np.float64)
    ecef = raw.get("antenna_positions")
    if ecef is None or np.shape(ecef) != enu.shape or not np.array_equal(enu_from_ecef_offsets(ecef, lat, lon), enu):
        ecef = ecef_offsets_from_enu(enu, lat, lon)
    uvw = getattr(uvd, "uvw_array", None)
    if uvw is None or len(uvw) != len(uvd.time_array):
        uvw = _uvw(uvd)
    i64 = np.int64
    derived = {
        "Nants_data": i64(uvd.Nants_data), "Nants_telescope": i64(uvd.Nants_telescope), "Nbls": i64(uvd.Nbls),
        "Nblts": i64(uvd.Nblts), "Nfreqs": i64(uvd.Nfreqs), "Npols": i64(uvd.Npols), "Nspws": i64(getattr(uvd, "Nspws", 1)),
        "Ntimes": i64(uvd.Ntimes), "latitude": np.float64(lat), "longitude": np.float64(lon), "altitude": np.float64(alt),
        "ant_1_array": np.asarray(uvd.ant_1_array, dtype=i64), "ant_2_array": np.asarray(uvd.ant_2_array, dtype=i64),
        "antenna_names": np.asarray([str(n).encode() for n in uvd.antenna_names]),
        "antenna_numbers": np.asarray(uvd.antenna_numbers), "antenna_positions": np.asarray(ecef, dtype=np.float64),
        "channel_width": np.asarray(uvd.channel_width, dtype=np.float64), "freq_array": np.asarray(uvd.freq_array, dtype=np.float64),
        "integration_time": np.asarray(uvd.integration_time, dtype=np.float64), "lst_array": np.asarray(uvd.lst_array, dtype=np.float64),
        "polarization_array": np.asarray(uvd.polarization_array, dtype=i64), "spw_array": np.asarray(getattr(uvd, "spw_array", [0]), dtype=i64),
        "telescope_name": str(uvd.telescope_name).encode(), "time_array": np.asarray(uvd.time_array, dtype=np.float64),
        "uvw_array": np.asarray(uvw, dtype=np.float64),
    }
    for name in _STRINGS:
        v = getattr(uvd, name, None)
        if v is None and not raw:
            v = _STRING_DEFAULTS[name] if name != "instrument" else str(uvd.telescope_name)
        if v is not None:
            derived[name] = str(v).encode()
    names = list(raw) if raw else list(_STANDARD)
    names = [n for n in names if n != "x_orientation"]
    if getattr(uvd, "x_orientation", None) is not None:
        derived["x_orientation"] = str(uvd.x_orientation).encode()
        names.append("x_orientation")
    header = {n: derived[n] if n in derived else raw[n] for n in names if n in derived or n in raw}
    for n in PER_BLT:
        if n in header and len(header[n]) != uvd.Nblts:
            raise ValueError(f"Header/{n} holds {len(header[n])} rows, the object {uvd.Nblts}")
    vis = np.asarray(uvd.data_array)
    vis = vis if vis.dtype in (np.complex64, np.complex128) else vis.astype(np.complex128)
    data = {"visdata": vis, "flags": np.asarray(uvd.flag_array, dtype=bool), "nsamples": np.asarray(uvd.nsample_array, dtype=np.float32)}
    hdf5.write(path, {"Header": header, "Data": data})
