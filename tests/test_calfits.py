"""The NumPy FITS subset (calamity_amd/fits.py) and the calfits mapping (calamity_amd/calfits.py): cards, blocks, axis
order and tables; round trips of gain objects of both array vintages; the driver's multi-file read; a foreign file
written by astropy in pyuvdata's layout (tests/golden/calfits/); and, where an interpreter with astropy is installed,
our files opened by astropy."""
import copy
import glob
import importlib.util
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from calamity_amd import cal_utils, calfits, calibration, fits, uvcompat, uvh5

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calfits")
FOREIGN = os.path.join(GOLDEN, "foreign_gain.calfits")
HERA_XYZ = np.array([5109342.76037543, 2005241.90402741, -3239939.46926407])


def _generator():
    spec = importlib.util.spec_from_file_location("make_calfits", os.path.join(GOLDEN, "make_calfits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the FITS layer -------------------------------------------------------------------------------------------------
def test_string_cards():
    card = fits.format_card("OBJECT", "it's", "a comment")
    assert len(card) == 1 and len(card[0]) == 80
    assert card[0].startswith("OBJECT  = 'it''s   ' / a comment")  # (the escaped text padded to 8)
    assert fits.format_card("SHORT", "ab")[0].startswith("SHORT   = 'ab      '")
    h = fits.Header.parse("".join(card + fits.format_card("END")).encode())
    assert h["OBJECT"] == "it's" and h.comment("OBJECT") == "a comment"
    # a long string with quotes takes CONTINUE cards ending in '&', and reads back whole
    long = " ".join(f"part {n} 'quoted'" for n in range(20))
    cards = fits.format_card("LONGSTR", long)
    assert len(cards) > 2 and all(len(c) == 80 for c in cards)
    assert all(c.startswith("CONTINUE  '") for c in cards[1:])
    assert all(c.rstrip().endswith("&'") for c in cards[:-1])
    h = fits.Header.parse(("".join(cards) + "END".ljust(80)).encode())
    assert h["LONGSTR"] == long and h.keys() == ["LONGSTR"]
    # an empty string, leading spaces kept, trailing ones not significant
    for s, back in (("", ""), ("  lead", "  lead"), ("trail   ", "trail")):
        assert fits.Header.parse((fits.format_card("S", s)[0] + "END".ljust(80)).encode())["S"] == back
    with pytest.raises(ValueError, match="printable ASCII"):
        fits.format_card("S", "café")


def test_number_and_logical_cards():
    for v in (True, False):
        card = fits.format_card("FLAG", v)[0]
        assert card[29] == ("T" if v else "F") and card[10:29].strip() == ""
    card = fits.format_card("NAXIS1", -12345)[0]
    assert card[:30] == "NAXIS1  =               -12345"
    values = [0.0, -0.1, 1e16, 6.02214076e23, -1.5e-300, 2459122.583513333, -np.pi, 5e-324, 100000000.0, 1.7976931348623157e308]
    cards = [fits.format_card(f"F{n}", v)[0] for n, v in enumerate(values)]
    for c in cards:
        s = c[10:].split("/")[0].strip()
        assert "e" not in s and ("." in s or "E" in s)
        if len(s) <= 20:
            assert c[29] != " " and c[30] == " "  # right-justified to column 30
    h = fits.Header.parse(("".join(cards) + "END".ljust(80)).encode())
    for n, v in enumerate(values):
        assert struct.pack("<d", h[f"F{n}"]) == struct.pack("<d", v)  # bit for bit
    # numbers written by other tools: D exponents, a leading "+", an undefined value, integers
    raw = ["A       =               1.5D-3", "B       =                +2.50", "C       =                      / undefined",
           "D       =                   42 / an int"]
    h = fits.Header.parse(("".join(c.ljust(80) for c in raw) + "END".ljust(80)).encode())
    assert h["A"] == 1.5e-3 and h["B"] == 2.5 and h["C"] is None and h["D"] == 42 and isinstance(h["D"], int)
    assert h.comment("C") == "undefined"
    with pytest.raises(ValueError):
        fits.format_card("BAD", float("nan"))
    with pytest.raises(ValueError, match="keyword"):
        fits.format_card("TOOLONGKEY", 1)


def test_history_cards():
    line = "".join(chr(ord("a") + n % 26) for n in range(100))
    cards = fits.format_card("HISTORY", line)
    assert len(cards) == 2 and [c[:8] for c in cards] == ["HISTORY "] * 2
    assert cards[0][8:] == line[:72] and cards[1][8:].rstrip() == line[72:]
    h = fits.Header.parse(("".join(cards + fits.format_card("COMMENT", "note")) + "END".ljust(80)).encode())
    assert h.commentary("HISTORY") == [line[:72], line[72:]] and h.commentary("COMMENT") == ["note"]
    with pytest.raises(ValueError, match="END"):
        fits.Header.parse("".join(cards).encode())


def _hdu_starts(path):
    raw = open(path, "rb").read()
    starts = [0] + [i for i in range(0, len(raw), 80) if raw[i:i + 9] == b"XTENSION="]
    return raw, starts


def test_blocks_padding_and_axis_order(tmp_path):
    path = str(tmp_path / "t.fits")
    rng = np.random.default_rng(0)
    images = {"F8": rng.standard_normal((2, 3, 5)), "F4": rng.standard_normal((7, 3)).astype(np.float32),
              "I2": np.arange(-6, 6, dtype=np.int16).reshape(3, 4), "I4": np.arange(-12, 12, dtype=np.int32).reshape(2, 3, 4),
              "I8": np.arange(5, dtype=np.int64) * -(2 ** 40), "U1": np.arange(250, 256, dtype=np.uint8)}
    hdus = [fits.image_hdu(images["F8"], [("MYKEY", "value")], primary=True)]
    hdus += [fits.image_hdu(a, name=k) for k, a in images.items() if k != "F8"]
    fits.write(path, hdus)
    raw, starts = _hdu_starts(path)
    assert len(raw) % fits.BLOCK == 0 and len(starts) == len(images)
    assert all(s % fits.BLOCK == 0 for s in starts)
    f = fits.open(path)
    for hdu, start in zip(f, starts):
        assert hdu._offset % fits.BLOCK == 0 and hdu._offset > start
        head = raw[start:hdu._offset]
        end = head.index(b"END     ")
        assert set(head[end + 3:]) == {ord(" ")}  # headers are padded with spaces
        stop = hdu._offset + hdu.nbytes
        assert set(raw[stop:fits._padded(stop)]) <= {0}  # data with zero bytes
    for hdu, (k, a) in zip(f, images.items()):
        # FITS axes are reversed: NAXIS1 is the last NumPy axis, and the bytes are the C-order big-endian array
        assert hdu.fits_shape == a.shape[::-1]
        assert [hdu.header[f"NAXIS{i + 1}"] for i in range(a.ndim)] == list(a.shape[::-1])
        assert raw[hdu._offset:hdu._offset + a.nbytes] == a.astype(a.dtype.newbyteorder(">")).tobytes()
        assert hdu.data is not None and hdu.data.dtype == a.dtype and np.array_equal(hdu.data, a)
    assert f[0].header["MYKEY"] == "value" and f["I2"].kind == "IMAGE" and f[0].kind == "PRIMARY"
    assert f[0].header["EXTEND"] is True and f[0].header["BITPIX"] == -64


def test_bintable(tmp_path):
    path = str(tmp_path / "t.fits")
    names = ["ANT0", "it's", "", "HH10", "12345678"]
    xyz = np.arange(15.0).reshape(5, 3) * -1.25
    cols = [("ANTNAME", "8A", names), ("ANTXYZ", "3D", xyz), ("ANTARR", "D", [0.0, 1.0, 2.0, -1.0, -1.0]),
            ("OK", "L", [True, False, True, True, False]), ("J", "J", [1, -2, 3, -4, 5]), ("K", "2K", np.arange(10).reshape(5, 2) - 2 ** 40),
            ("E", "E", np.linspace(0, 1, 5)), ("B", "B", [0, 1, 2, 254, 255]), ("I", "I", [-32768, 0, 1, 2, 32767])]
    fits.write(path, [fits.image_hdu(None, primary=True), fits.bintable_hdu(cols, name="ANTENNAS")])
    f = fits.open(path)
    t = f["ANTENNAS"]
    assert t.kind == "BINTABLE" and t.nrows == 5 and t.header["NAXIS1"] == 8 + 24 + 8 + 1 + 4 + 16 + 4 + 1 + 2
    assert [t.header[f"TFORM{n}"] for n in range(1, 10)] == [c[1] for c in cols]
    d = t.data
    assert list(d["ANTNAME"]) == names and d["ANTXYZ"].shape == (5, 3) and np.array_equal(d["ANTXYZ"], xyz)
    assert np.array_equal(d["ANTARR"], cols[2][2]) and d["OK"].dtype == bool and list(d["OK"]) == cols[3][2]
    assert list(d["J"]) == cols[4][2] and np.array_equal(d["K"], cols[5][2])
    assert np.array_equal(d["E"], np.linspace(0, 1, 5).astype(np.float32)) and list(d["B"]) == cols[7][2] and list(d["I"]) == cols[8][2]
    assert f[0].data is None and f[0].header["NAXIS"] == 0
    with pytest.raises(ValueError, match="longer than 8"):
        fits.bintable_hdu([("ANTNAME", "8A", ["123456789"])])


def _raw_file(path, units):
    """[(cards, data bytes)] -> a FITS file written card by card (for inputs the writer never makes)."""
    with open(path, "wb") as f:
        for cards, data in units:
            f.write(fits.Header(cards).tobytes())
            f.write(data + b"\0" * (fits._padded(len(data)) - len(data)))


PRIMARY0 = [("SIMPLE", True), ("BITPIX", 8), ("NAXIS", 0), ("EXTEND", True)]


def _table_cards(extra=(), tform="D", pcount=0):
    return [("XTENSION", "BINTABLE"), ("BITPIX", 8), ("NAXIS", 2), ("NAXIS1", 8), ("NAXIS2", 1), ("PCOUNT", pcount),
            ("GCOUNT", 1), ("TFIELDS", 1), ("TTYPE1", "X"), ("TFORM1", tform)] + list(extra)


@pytest.mark.parametrize("case, match", [
    ("groups", "random groups"), ("vla", "variable-length"), ("heap", "heap"), ("tscal", "TSCAL1"), ("tzero", "TZERO1"),
    ("ascii", "'TABLE'"), ("bscale", "BSCALE"), ("bitpix", "BITPIX = 24"), ("code", "column type 'X'"),
    ("truncated", "truncated"), ("partial", "truncated"), ("width", "NAXIS1 = 8"), ("notfits", "not a FITS file"),
])
def test_unsupported_inputs_raise(tmp_path, case, match):
    path = str(tmp_path / f"{case}.fits")
    row = b"\0" * 8
    if case == "groups":
        _raw_file(path, [([("SIMPLE", True), ("BITPIX", -32), ("NAXIS", 2), ("NAXIS1", 0), ("NAXIS2", 1), ("GROUPS", True),
                           ("PCOUNT", 0), ("GCOUNT", 1)], b"\0" * 4)])
    elif case == "vla":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards(tform="1PJ(4)"), row)])
    elif case == "heap":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards(pcount=16), row + b"\0" * 16)])
    elif case == "tscal":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards([("TSCAL1", 2.0)]), row)])
    elif case == "tzero":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards([("TZERO1", 32768)], tform="I"), b"\0" * 2)])
    elif case == "ascii":
        _raw_file(path, [(PRIMARY0, b""), ([("XTENSION", "TABLE"), ("BITPIX", 8), ("NAXIS", 2), ("NAXIS1", 8), ("NAXIS2", 1),
                                            ("PCOUNT", 0), ("GCOUNT", 1), ("TFIELDS", 1), ("TFORM1", "F8.3")], row)])
    elif case == "bscale":
        _raw_file(path, [([("SIMPLE", True), ("BITPIX", 16), ("NAXIS", 1), ("NAXIS1", 4), ("BSCALE", 2.0), ("BZERO", 0.0)], row)])
    elif case == "bitpix":
        _raw_file(path, [([("SIMPLE", True), ("BITPIX", 24), ("NAXIS", 1), ("NAXIS1", 2)], b"\0" * 6)])
    elif case == "code":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards(tform="64X"), row)])
    elif case == "width":
        _raw_file(path, [(PRIMARY0, b""), (_table_cards(tform="J"), row)])
    elif case in ("truncated", "partial"):
        fits.write(path, [fits.image_hdu(np.zeros((40, 40)), primary=True)])
        raw = open(path, "rb").read()
        open(path, "wb").write(raw[:fits.BLOCK + 1000] if case == "truncated" else raw[:fits.BLOCK - 80])
    elif case == "notfits":
        open(path, "wb").write(b"SIMPLE  =                    F".ljust(fits.BLOCK))
    with pytest.raises(ValueError, match=match):
        f = fits.open(path)
        for hdu in f:
            hdu.data


# ---- the calfits layer ----------------------------------------------------------------------------------------------
def make_gains(ntimes, njones, future_shapes, telescope_xyz=None, seed=0):
    """A gain object of 4 of the telescope's 6 antennas, random gains, flags and quality, from a SimpleUVData."""
    rng = np.random.default_rng(seed)
    antpos = rng.uniform(-50, 50, (6, 3)) * np.array([1.0, 1.0, 0.01])
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    freqs = 120e6 + np.arange(24) * 97656.25
    times = 2459122.25 + np.arange(ntimes) * 10.0 / 86400.0
    uvd = uvcompat.SimpleUVData(antpos, pairs, freqs, times, pols=[-5, -6][:njones], x_orientation="east", future_shapes=future_shapes)
    if telescope_xyz is not None:
        uvd.telescope_location = np.asarray(telescope_xyz, dtype=np.float64)
        uvd.telescope_name = "HERA"
    g = cal_utils.blank_uvcal_from_uvdata(uvd)
    shape = g.gain_array.shape
    g.gain_array = g.gain_array + 0.05 * rng.standard_normal(shape) + 0.05j * rng.standard_normal(shape)
    g.flag_array = rng.random(shape) < 0.1
    g.quality_array = rng.random(shape)
    g.history = "made by make_gains\n" + " ".join(["a long history line that takes more than one card"] * 3)
    return uvd, g


def assert_same_gains(back, g, exact_positions=True):
    for name in ("gain_array", "flag_array", "quality_array"):
        a, b = getattr(back, name), getattr(g, name)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), name
    assert np.max(np.abs(back.time_array - g.time_array)) <= 1e-9
    assert back.freq_array.shape == np.shape(g.freq_array) and np.allclose(back.freq_array, g.freq_array, rtol=0, atol=1e-6)
    for name in ("ant_array", "jones_array", "antenna_numbers", "spw_array", "lst_array", "telescope_location"):
        assert np.array_equal(getattr(back, name), getattr(g, name)), name
    for name in ("Nfreqs", "Njones", "Ntimes", "Nspws", "Nants_data", "Nants_telescope", "antenna_names", "telescope_name",
                 "integration_time", "channel_width", "x_orientation", "gain_convention", "cal_style", "cal_type", "time_range"):
        assert getattr(back, name) == getattr(g, name), name
    assert back.history.replace("\n", "") == g.history.replace("\n", "")
    if exact_positions:
        assert np.array_equal(back.antenna_positions, g.antenna_positions)
    else:
        assert np.allclose(back.antenna_positions, g.antenna_positions, rtol=0, atol=1e-8)


@pytest.mark.parametrize("future_shapes", [False, True], ids=["spw_axis", "no_spw_axis"])
@pytest.mark.parametrize("ntimes, njones", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_round_trip(tmp_path, ntimes, njones, future_shapes):
    uvd, g = make_gains(ntimes, njones, future_shapes)
    assert g.Nants_data == 4 < g.Nants_telescope == 6
    path = str(tmp_path / "g.calfits")
    g.write_calfits(path)
    assert open(path, "rb").read(30) == fits.SIMPLE_CARD
    back = uvcompat.read_container(path)
    assert isinstance(back, uvcompat.SimpleUVCal)
    assert_same_gains(back, g)
    # the pyuvdata method name fills an empty object
    obj = uvcompat.SimpleUVCal()
    obj.read_calfits(path)
    assert_same_gains(obj, g)
    # the layout of pyuvdata's writer
    f = fits.open(path)
    h = f[0].header
    assert f[0].data.shape == (4, 1, 24, ntimes, njones, 4) and f[0].header["BITPIX"] == -64
    assert [h[f"CTYPE{n}"] for n in range(1, 7)] == ["Narrays", "JONES", "TIME", "FREQS", "IF", "ANTAXIS"]
    assert h["CDELT2"] == -1 and h["CRVAL2"] == -5
    assert h["CDELT3"] == (10.0 / 86400.0 if ntimes == 1 else h["CDELT3"]) and h["SPWAXIS"] is (not future_shapes)
    ant = f["ANTENNAS"].data
    assert list(ant["ANTARR"]) == [0, 1, 2, 3, -1, -1] and list(ant["ANTINDEX"]) == list(range(6)) and ant["ANTXYZ"].shape == (6, 3)
    assert [f["ANTENNAS"].header[f"TFORM{n}"] for n in range(1, 5)] == ["8A", "D", "D", "3D"]
    # gains read from the file act as the in-memory ones
    for t in np.unique(uvd.time_array):
        for pol in uvd.get_pols():
            for a, b in zip(calibration.tensorize_gains(back, pol, t, np.float64), calibration.tensorize_gains(g, pol, t, np.float64)):
                assert np.array_equal(a, b)
    uvd.data_array = uvd.data_array + 1.0 + 0.5j
    assert np.array_equal(cal_utils.apply_gains(uvd, back).data_array, cal_utils.apply_gains(uvd, g).data_array)
    # existing files are only replaced on request
    with pytest.raises(IOError):
        g.write_calfits(path)
    g.write_calfits(path, clobber=True)


def test_round_trip_at_a_telescope(tmp_path):
    """A real telescope location: ENU -> ECEF offsets -> ENU through uvh5.py's rotations; a total quality array."""
    _, g = make_gains(3, 2, False, telescope_xyz=HERA_XYZ)
    g.total_quality_array = np.random.default_rng(3).random((1, g.Nfreqs, g.Ntimes, g.Njones))
    path = str(tmp_path / "g.calfits")
    g.write_calfits(path)
    back = calfits.read_calfits(path)
    assert_same_gains(back, g, exact_positions=False)
    assert np.array_equal(back.total_quality_array, g.total_quality_array)
    lat, lon, alt = uvh5.lat_lon_alt_from_ecef(HERA_XYZ)
    h = fits.open(path)[0].header
    assert (h["LAT"], h["LON"], h["ALT"]) == (lat, lon, alt) and abs(lat + 30.72) < 0.01 and abs(lon - 21.43) < 0.01
    xyz = fits.open(path)["ANTENNAS"].data["ANTXYZ"]
    assert np.allclose(xyz, uvh5.ecef_offsets_from_enu(g.antenna_positions, lat, lon), rtol=0, atol=1e-9)
    _, g4 = make_gains(2, 1, True)
    g4.total_quality_array = np.ones((g4.Nfreqs, g4.Ntimes, g4.Njones))
    g4.write_calfits(path, clobber=True)
    assert np.array_equal(calfits.read_calfits(path).total_quality_array, g4.total_quality_array)


def test_writer_refusals(tmp_path):
    path = str(tmp_path / "g.calfits")
    _, g = make_gains(3, 2, False)
    bad = copy.deepcopy(g)
    bad.time_array = bad.time_array + np.array([0.0, 0.0, 1e-4])
    with pytest.raises(ValueError, match="times are not evenly spaced"):
        bad.write_calfits(path)
    _, g1 = make_gains(1, 1, True)
    bad = copy.deepcopy(g1)
    bad.freq_array = bad.freq_array.copy()
    bad.freq_array[5] += 1.0
    with pytest.raises(ValueError, match="frequencies are not evenly spaced"):
        bad.write_calfits(path)
    bad = copy.deepcopy(g)
    bad.jones_array = np.array([-5, -7])
    bad.write_calfits(path)  # (two values are always evenly spaced)
    os.remove(path)
    _, g3 = make_gains(1, 1, False)
    g3.jones_array = np.array([-5, -6, -8])
    g3.gain_array = np.ones(g3.gain_array.shape[:-1] + (3,), dtype=complex)
    g3.flag_array = np.zeros(g3.gain_array.shape, dtype=bool)
    g3.quality_array = np.zeros(g3.gain_array.shape)
    with pytest.raises(ValueError, match="jones values are not evenly spaced"):
        g3.write_calfits(path)
    for attr, value, match in (("cal_type", "delay", "gain-type"), ("Nspws", 2, "single-spw")):
        bad = copy.deepcopy(g)
        setattr(bad, attr, value)
        with pytest.raises(ValueError, match=match):
            bad.write_calfits(path)
    assert not os.path.exists(path)


def _split(g, keep):
    """The gain object restricted to the times ``keep`` (a boolean mask)."""
    out = copy.deepcopy(g)
    tax = np.ndim(g.gain_array) - 2
    for name in ("gain_array", "flag_array", "quality_array"):
        setattr(out, name, np.compress(keep, getattr(g, name), axis=tax))
    out.time_array, out.lst_array = g.time_array[keep], g.lst_array[keep]
    out.Ntimes = int(np.sum(keep))
    out.time_range = (out.time_array.min() - out.integration_time / 2.0, out.time_array.max() + out.integration_time / 2.0)
    return out


@pytest.mark.parametrize("future_shapes", [False, True], ids=["spw_axis", "no_spw_axis"])
def test_read_several_files(tmp_path, future_shapes):
    _, g = make_gains(3, 2, future_shapes)
    paths = [str(tmp_path / n) for n in ("a.calfits", "b.calfits", "c.calfits")]
    _split(g, np.array([False, True, True])).write_calfits(paths[0])  # (later times first: the result is time-ordered)
    _split(g, np.array([True, False, False])).write_calfits(paths[1])
    whole = calfits.read_calfits([paths[0], paths[1]])
    assert_same_gains(whole, g)
    obj = uvcompat.SimpleUVCal()
    obj.read_calfits(paths[:2])
    assert_same_gains(obj, g)
    if not _has_pyuvdata():
        assert_same_gains(calibration._read_uvcal(paths[:2]), g)
    # a shared time, or other frequencies, antennas or jones, are refused
    _split(g, np.array([True, True, False])).write_calfits(paths[2])
    with pytest.raises(ValueError, match="holds a time"):
        calfits.read_calfits([paths[0], paths[2]])
    other = _split(g, np.array([True, False, False]))
    other.freq_array = other.freq_array + 1e3
    other.write_calfits(paths[2], clobber=True)
    with pytest.raises(ValueError, match="frequencies differ"):
        calfits.read_calfits([paths[0], paths[2]])
    other = _split(g, np.array([True, False, False]))
    other.ant_array = other.ant_array + 1
    other.write_calfits(paths[2], clobber=True)
    with pytest.raises(ValueError, match="antennas differ"):
        calfits.read_calfits([paths[0], paths[2]])
    other = _split(g, np.array([True, False, False]))
    other.jones_array = np.array([-7, -8])
    other.write_calfits(paths[2], clobber=True)
    with pytest.raises(ValueError, match="jones values differ"):
        calfits.read_calfits([paths[0], paths[2]])


def _has_pyuvdata():
    try:
        import pyuvdata  # noqa: F401
    except ImportError:
        return False
    return True


def test_read_container_reads_calfits_and_archives(tmp_path):
    _, g = make_gains(3, 1, False)
    fitsfile, archive = str(tmp_path / "g.calfits"), str(tmp_path / "old.calfits")
    g.write_calfits(fitsfile)
    uvcompat._write_container(g, archive, False, "uvcal")  # the gain files earlier versions wrote
    assert open(archive, "rb").read(2) == b"PK"
    for path in (fitsfile, archive):
        back = uvcompat.read_container(path)
        assert isinstance(back, uvcompat.SimpleUVCal)
        for name in ("gain_array", "flag_array", "quality_array", "ant_array", "jones_array"):
            assert np.array_equal(getattr(back, name), getattr(g, name))
    if not _has_pyuvdata():
        for path in (fitsfile, archive):
            assert np.array_equal(calibration._read_uvcal(path).gain_array, g.gain_array)
        assert np.array_equal(calibration._read_uvcal([fitsfile]).gain_array, g.gain_array)


# ---- a file written by another FITS implementation -----------------------------------------------------------------
def test_foreign_fixture():
    """tests/golden/calfits/foreign_gain.calfits (astropy, pyuvdata's layout, no SPWAXIS / LSTS): every value."""
    m = _generator()
    gain, flag, quality, total = m.arrays()
    g = uvcompat.read_container(FOREIGN)
    assert isinstance(g, uvcompat.SimpleUVCal)
    # no SPWAXIS keyword: the array shapes of pyuvdata >= 3
    assert g.gain_array.shape == (3, m.NFREQS, m.NTIMES, m.NJONES) and g.freq_array.shape == (m.NFREQS,)
    assert g.gain_array.dtype == np.complex128 and np.array_equal(g.gain_array, gain)
    assert g.flag_array.dtype == bool and np.array_equal(g.flag_array, flag) and flag.any() and not flag.all()
    assert np.array_equal(g.quality_array, quality) and np.array_equal(g.total_quality_array, total)
    assert list(g.ant_array) == m.ANT_ARRAY and list(g.antenna_numbers) == m.ANTENNA_NUMBERS
    assert g.antenna_names == m.ANTENNA_NAMES and g.Nants_telescope == 4 and g.Nants_data == 3
    assert list(g.jones_array) == [-5, -6] and g.Njones == 2 and g.Nfreqs == m.NFREQS and g.Ntimes == m.NTIMES
    assert np.allclose(g.time_array, m.TIME0 + np.arange(m.NTIMES) * m.INTTIME / 86400.0, rtol=0, atol=1e-9)
    assert np.array_equal(g.freq_array, m.FREQ0 + np.arange(m.NFREQS) * m.DFREQ)
    assert g.integration_time == m.INTTIME and g.channel_width == m.DFREQ and g.time_range == m.TIME_RANGE
    assert g.telescope_name == "HERA" and g.x_orientation == "east" and g.gain_convention == "divide"
    assert g.cal_type == "gain" and g.cal_style == "redundant"
    assert np.array_equal(g.telescope_location, m.ARRAY_XYZ)
    assert np.allclose(uvh5.ecef_offsets_from_enu(g.antenna_positions, m.LAT, m.LON), m.antenna_xyz(), rtol=0, atol=1e-9)
    # astropy splits the 100-character history line over two cards; the reader joins cards with newlines
    assert g.history.replace("\n", "") == "".join(m.HISTORY)
    # no LSTS extension: mean sidereal time from the times and the longitude (2020-09-30 18:00 UT at 21.43 deg E is
    # about 20h03m of LST)
    assert g.lst_array.shape == (m.NTIMES,) and abs(g.lst_array[0] - 20.05 / 24.0 * 2.0 * np.pi) < 0.01
    assert np.allclose(np.diff(g.lst_array), 2.0 * np.pi * 1.00273781191135448 * m.INTTIME / 86400.0, rtol=1e-6)
    # it writes back and re-reads unchanged (now with the vintage keyword and the LSTs stored)
    assert g.spw_array.tolist() == [0]


def test_foreign_fixture_writes_back(tmp_path):
    g = calfits.read_calfits(FOREIGN)
    path = str(tmp_path / "again.calfits")
    g.write_calfits(path)
    back = calfits.read_calfits(path)
    assert_same_gains(back, g, exact_positions=False)
    assert np.array_equal(back.total_quality_array, g.total_quality_array)
    assert fits.open(path)[0].header["SPWAXIS"] is False


def test_lst_from_jd():
    # J2000.0 (2000-01-01 12:00 UT): GMST 18h41m50.548s (the ERA + polynomial value, UT1 = UTC)
    assert abs(calfits.lst_from_jd(2451545.0, 0.0) - (18 + 41 / 60 + 50.548 / 3600) / 24 * 2 * np.pi) < 1e-6
    east = calfits.lst_from_jd(2451545.0, 90.0) - calfits.lst_from_jd(2451545.0, 0.0)
    assert abs((east - np.pi / 2 + np.pi) % (2 * np.pi) - np.pi) < 1e-12


# ---- cross-check with astropy, where an interpreter has it --------------------------------------------------------
_ASTROPY_DUMP = r"""
import json, sys
import numpy as np
np.asscalar = lambda a: a.item()
np.alen = len
from astropy.io import fits
with fits.open(sys.argv[1]) as f:
    f.verify("exception")
    h = f[0].header
    t = f["ANTENNAS"].data
    out = {"names": [x.name for x in f], "shape": list(f[0].data.shape), "data": f[0].data.astype("<f8").ravel().tolist(),
           "ctype": [h["CTYPE%d" % n] for n in range(1, 7)], "history": [str(x) for x in h["HISTORY"]],
           "tmerange": h["TMERANGE"], "crval3": h["CRVAL3"], "cdelt3": h["CDELT3"],
           "formats": [c.format for c in f["ANTENNAS"].columns],
           "antname": [str(x) for x in t["ANTNAME"]], "antindex": t["ANTINDEX"].tolist(), "antarr": t["ANTARR"].tolist(),
           "antxyz": t["ANTXYZ"].tolist()}
print(json.dumps(out))
"""


def astropy_python():
    cands = [sys.executable, shutil.which("python3.9"), "/opt/conda/bin/python3.9"]
    cands += sorted(p for p in glob.glob("/opt/conda/bin/python3.*") if p.rsplit(".", 1)[-1].isdigit())
    for exe in dict.fromkeys(c for c in cands if c and os.path.exists(c)):
        r = subprocess.run([exe, "-c", "import numpy as np; np.asscalar = lambda a: a.item(); np.alen = len; import astropy.io.fits"],
                           capture_output=True, timeout=120)
        if r.returncode == 0:
            return exe
    pytest.skip("no interpreter with a working astropy.io.fits is installed")


def test_astropy_opens_our_files(tmp_path):
    exe = astropy_python()
    _, g = make_gains(3, 2, False, telescope_xyz=HERA_XYZ)
    g.total_quality_array = np.zeros((1, g.Nfreqs, g.Ntimes, g.Njones))
    path = str(tmp_path / "g.calfits")
    g.write_calfits(path)
    r = subprocess.run([exe, "-c", _ASTROPY_DUMP, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    ours = fits.open(path)
    assert got["names"] == ["PRIMARY", "ANTENNAS", "TOTQLTY", "LSTS"]
    assert got["shape"] == [4, 1, g.Nfreqs, 3, 2, 4] and np.array_equal(np.asarray(got["data"]), ours[0].data.ravel())
    assert got["ctype"] == ["Narrays", "JONES", "TIME", "FREQS", "IF", "ANTAXIS"]
    assert got["crval3"] == g.time_array[0] and got["cdelt3"] == ours[0].header["CDELT3"]
    assert "".join(got["history"]) == g.history.replace("\n", "")
    assert got["tmerange"] == ",".join(repr(float(t)) for t in g.time_range)
    assert got["formats"] == ["8A", "D", "D", "3D"]
    ant = ours["ANTENNAS"].data
    assert got["antname"] == list(ant["ANTNAME"]) == g.antenna_names
    assert got["antindex"] == ant["ANTINDEX"].tolist() and got["antarr"] == [0, 1, 2, 3, -1, -1]
    assert np.array_equal(np.asarray(got["antxyz"]), ant["ANTXYZ"])
