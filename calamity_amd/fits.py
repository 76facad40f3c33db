"""The subset of FITS that calfits files use, read and written in pure Python and NumPy (no astropy, no cfitsio).

A file is a sequence of HDUs (header + data unit), each starting on a 2880-byte block: headers are 80-character
cards padded with spaces, data units big-endian and padded with zero bytes.

Headers: fixed-format value cards (strings quoted, ``''`` for a quote, padded to 8 characters; logicals ``T``/``F`` and
numbers right-justified to column 30; floats written with ``repr``, so a float64 reads back bit for bit), ``/ comment``
after a value, ``HISTORY`` / ``COMMENT`` cards, ``END``.  The reader follows the ``CONTINUE`` long-string convention
(``&`` at the end of a string continues it); the writer uses it for strings longer than one card and splits history
lines over 72-character ``HISTORY`` cards.

HDUs: the primary HDU, ``IMAGE`` extensions (BITPIX 8/16/32/64/-32/-64; BSCALE / BZERO only as 1 / 0) and ``BINTABLE``
extensions with TFORM codes ``L A B I J K E D`` and repeat counts.  FITS lists axes fastest first: NAXIS1 is the last
NumPy axis.  Opening a file parses the headers only; a data unit is read when ``HDU.data`` is asked for.

Anything else -- random groups, ASCII tables, variable-length arrays (``P`` / ``Q``), heaps, TSCALn / TZEROn / TDIMn,
scaled images, a truncated file -- raises ``ValueError`` naming it: this module never guesses.
"""
import builtins
import os
import re

import numpy as np

BLOCK = 2880
CARD = 80
SIMPLE_CARD = b"SIMPLE  =                    T"  # the first 30 bytes of every standard FITS file

_BITPIX = {8: "u1", 16: ">i2", 32: ">i4", 64: ">i8", -32: ">f4", -64: ">f8"}
_IMAGE_BITPIX = {("u", 1): 8, ("i", 2): 16, ("i", 4): 32, ("i", 8): 64, ("f", 4): -32, ("f", 8): -64}  # (BITPIX 8 is unsigned)
_TFORM = {"L": "i1", "B": "u1", "I": ">i2", "J": ">i4", "K": ">i8", "E": ">f4", "D": ">f8"}  # (+ "A": "S<repeat>")
_TFORM_RE = re.compile(r"^\s*(\d*)([A-Z])(.*)$")
_INT_RE = re.compile(r"^[+-]?\d+$")
_FLOAT_RE = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([ED][+-]?\d+)?$")
_KEY_RE = re.compile(r"^[A-Z0-9_-]{0,8}$")
_COMMENTARY = ("HISTORY", "COMMENT", "")


def _padded(n):
    return -(-n // BLOCK) * BLOCK


# ---- cards ---------------------------------------------------------------------------------------------------------
def _check_text(s, what):
    if any(not (32 <= ord(ch) <= 126) for ch in s):
        raise ValueError(f"FITS: {what} {s!r} holds characters outside printable ASCII")


def _number(v):
    if isinstance(v, (bool, np.bool_)):
        return "T" if v else "F"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = float(v)
    if not np.isfinite(v):
        raise ValueError(f"FITS: a header value cannot be {v}")
    s = repr(v).upper()  # shortest string that reads back as the same float64
    return s if ("." in s or "E" in s) else s + ".0"


def _string_pieces(s, first_room):
    """Split ``s`` into escaped pieces that fit ``first_room`` characters between the quotes on the first card and 67
    on every CONTINUE card (each piece but the last is followed by ``&``)."""
    pieces, cur, room = [], "", first_room
    for ch in s:
        e = "''" if ch == "'" else ch
        if len(cur) + len(e) > room - 1:  # (room for the "&")
            pieces.append(cur + "&")
            cur, room = "", 67
        cur += e
    pieces.append(cur)
    return pieces


def format_card(key, value=None, comment=None):
    """One keyword -> the 80-character card(s) it takes (several for a long string, via CONTINUE)."""
    key = key.upper()
    if not _KEY_RE.match(key):
        raise ValueError(f"FITS: keyword {key!r} is not 1-8 characters of A-Z 0-9 _ -")
    if key in _COMMENTARY:
        text = "" if value is None else str(value)
        _check_text(text, "commentary text")
        return [f"{key:<8}{text[i:i + 72]}".ljust(CARD) for i in range(0, max(len(text), 1), 72)]
    comment = None if comment is None else str(comment)
    if comment is not None:
        _check_text(comment, "comment")
    if isinstance(value, str):
        _check_text(value, "string")
        pieces = _string_pieces(value, 68)
        cards = []
        for n, p in enumerate(pieces):
            body = f"'{p:<8}'" if len(pieces) == 1 else f"'{p}'"
            cards.append(f"{key:<8}= {body}" if n == 0 else f"CONTINUE  {body}")
        if comment is not None and len(cards[-1]) + 3 + len(comment) <= CARD:
            cards[-1] += f" / {comment}"
        return [c.ljust(CARD) for c in cards]
    if value is None:
        card = f"{key:<8}= {'':20}"
    else:
        card = f"{key:<8}= {_number(value):>20}"
    if len(card) > CARD:
        raise ValueError(f"FITS: the value of {key} does not fit one card")
    if comment is not None:
        card = (card + f" / {comment}")[:CARD]
    return [card.ljust(CARD)]


def _parse_string(text):
    """``'...'...`` (starting at the quote) -> (string, rest of the card after the closing quote)."""
    out, i = [], 1
    while True:
        j = text.find("'", i)
        if j < 0:
            raise ValueError(f"FITS: unterminated string in card value {text!r}")
        out.append(text[i:j])
        if text[j + 1:j + 2] == "'":
            out.append("'")
            i = j + 2
            continue
        return "".join(out).rstrip(), text[j + 1:]


def _parse_value(key, text):
    """The value field of a card (columns 11-80) -> (value, comment)."""
    stripped = text.lstrip()
    if stripped.startswith("'"):
        value, rest = _parse_string(stripped)
    else:
        cut = stripped.find("/")
        value, rest = (stripped, "") if cut < 0 else (stripped[:cut], stripped[cut:])
        value = value.strip()
        if value == "":
            value = None
        elif value in ("T", "F"):
            value = value == "T"
        elif _INT_RE.match(value):
            value = int(value)
        elif _FLOAT_RE.match(value):
            value = float(value.replace("D", "E"))
        else:
            raise ValueError(f"FITS: value {value!r} of {key} is not a string, logical, integer or real number")
    rest = rest.strip()
    if rest and not rest.startswith("/"):
        raise ValueError(f"FITS: unexpected text {rest!r} after the value of {key}")
    return value, (rest[1:].strip() if rest else None)


class Header:
    """An ordered list of (keyword, value, comment) cards; commentary cards (HISTORY, COMMENT, blank) keep their text
    as the value.  Indexing returns the first value of a keyword."""

    def __init__(self, cards=()):
        self.cards = []
        for c in cards:
            self.append(*c)

    def append(self, key, value=None, comment=None):
        self.cards.append((key.upper(), value, comment))

    def __contains__(self, key):
        return any(k == key for k, _, _ in self.cards)

    def __getitem__(self, key):
        for k, v, _ in self.cards:
            if k == key:
                return v
        raise KeyError(key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def comment(self, key):
        for k, _, c in self.cards:
            if k == key:
                return c
        raise KeyError(key)

    def commentary(self, key):
        """The texts of every ``key`` (HISTORY or COMMENT) card, in order."""
        return [v for k, v, _ in self.cards if k == key]

    def keys(self):
        return [k for k, _, _ in self.cards]

    def tobytes(self):
        lines = [line for k, v, c in self.cards for line in format_card(k, v, c)]
        lines.append("END".ljust(CARD))
        raw = "".join(lines).encode("ascii")
        return raw.ljust(_padded(len(raw)), b" ")

    @classmethod
    def parse(cls, raw):
        """Cards up to END (``raw``: a whole number of cards) -> Header."""
        h = cls()
        text = raw.decode("ascii")
        for i in range(0, len(text), CARD):
            card = text[i:i + CARD]
            key = card[:8].rstrip()
            if key == "END":
                return h
            if key == "CONTINUE" and card[8:10] != "= ":
                if not h.cards or not isinstance(h.cards[-1][1], str) or not h.cards[-1][1].endswith("&"):
                    raise ValueError("FITS: CONTINUE card without a preceding string ending in '&'")
                value, comment = _parse_value(key, card[8:])
                if not isinstance(value, str):
                    raise ValueError("FITS: CONTINUE card without a string value")
                k, v, c = h.cards[-1]
                h.cards[-1] = (k, v[:-1] + value, comment if comment is not None else c)
            elif card[8:10] == "= " and key not in _COMMENTARY:
                h.cards.append((key, *_parse_value(key, card[10:])))
            else:
                h.cards.append((key, card[8:].rstrip(), None))
        raise ValueError("FITS: header without an END card")


# ---- HDUs ----------------------------------------------------------------------------------------------------------
def _tform(code, col):
    m = _TFORM_RE.match(code)
    if not m:
        raise ValueError(f"FITS: cannot parse TFORM{col} = {code!r}")
    repeat, letter, extra = int(m.group(1) or 1), m.group(2), m.group(3).strip()
    if letter in ("P", "Q"):
        raise ValueError(f"FITS: TFORM{col} = {code!r}: variable-length arrays are not supported")
    if letter != "A" and letter not in _TFORM:
        raise ValueError(f"FITS: TFORM{col} = {code!r}: column type {letter!r} is not supported")
    if extra:
        raise ValueError(f"FITS: TFORM{col} = {code!r}: trailing {extra!r} is not supported")
    return repeat, letter


class HDU:
    """One header + data unit.  ``kind``: "PRIMARY", "IMAGE" or "BINTABLE"; ``data``: an array in NumPy axis order
    (images) or a dict column name -> array (tables, string columns as ``str`` arrays), read on first access."""

    def __init__(self, header, path=None, offset=None):
        self.header, self._path, self._offset = header, path, offset
        self._data = None
        if "SIMPLE" in header and header.keys()[0] == "SIMPLE":
            if header["SIMPLE"] is not True:
                raise ValueError("FITS: SIMPLE = F (a non-conforming file)")
            if header.get("GROUPS") is True or (header.get("NAXIS", 0) > 0 and header.get("NAXIS1") == 0):
                raise ValueError("FITS: random groups are not supported")
            self.kind = "PRIMARY"
        else:
            xt = str(header.get("XTENSION", "")).strip()
            if xt not in ("IMAGE", "BINTABLE"):
                raise ValueError(f"FITS: extension type XTENSION = {xt!r} is not supported")
            self.kind = xt
            if header.get("GCOUNT", 1) != 1:
                raise ValueError(f"FITS: GCOUNT = {header['GCOUNT']} (groups) is not supported")
            if header.get("PCOUNT", 0) != 0:
                raise ValueError(f"FITS: PCOUNT = {header['PCOUNT']}: " + ("a heap" if xt == "BINTABLE" else "parameters") + " is not supported")
        self.name = str(header.get("EXTNAME", "PRIMARY" if self.kind == "PRIMARY" else "")).strip()
        naxis = int(header.get("NAXIS", 0))
        self.fits_shape = tuple(int(header[f"NAXIS{i}"]) for i in range(1, naxis + 1))  # NAXIS1 first
        if self.kind == "BINTABLE":
            self._table_layout()
        else:
            bitpix = int(header["BITPIX"])
            if bitpix not in _BITPIX:
                raise ValueError(f"FITS: BITPIX = {bitpix} is not supported")
            if header.get("BSCALE", 1) != 1 or header.get("BZERO", 0) != 0:
                raise ValueError(f"FITS: scaled image data (BSCALE = {header.get('BSCALE', 1)}, BZERO = {header.get('BZERO', 0)}) are not supported")
            self._dtype = np.dtype(_BITPIX[bitpix])
            self.shape = self.fits_shape[::-1]
        nelem = int(np.prod(self.fits_shape)) if self.fits_shape else 0
        self.nbytes = nelem * (1 if self.kind == "BINTABLE" else self._dtype.itemsize)

    def _table_layout(self):
        h = self.header
        if int(h["BITPIX"]) != 8 or int(h["NAXIS"]) != 2:
            raise ValueError("FITS: a BINTABLE needs BITPIX = 8 and NAXIS = 2")
        nfields = int(h["TFIELDS"])
        for k in h.keys():
            for bad in ("TSCAL", "TZERO", "TDIM", "THEAP"):
                if k.startswith(bad) and k[len(bad):].isdigit() or k == bad:
                    raise ValueError(f"FITS: BINTABLE keyword {k} is not supported")
        names, formats, offsets, self.columns, off = [], [], [], [], 0
        for n in range(1, nfields + 1):
            repeat, letter = _tform(str(h[f"TFORM{n}"]), n)
            name = str(h.get(f"TTYPE{n}", f"COL{n}")).strip()
            if letter == "A":
                dt, width = np.dtype(f"S{repeat}"), repeat
            else:
                base = np.dtype(_TFORM[letter])
                dt, width = (np.dtype((base, (repeat,))) if repeat != 1 else base), repeat * base.itemsize
            names.append(name)
            formats.append(dt)
            offsets.append(off)
            self.columns.append((name, letter, repeat))
            off += width
        if off != self.fits_shape[0]:
            raise ValueError(f"FITS: BINTABLE columns take {off} bytes a row, NAXIS1 = {self.fits_shape[0]}")
        self._dtype = np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": off})
        self.nrows = self.fits_shape[1]

    @property
    def data(self):
        if self._data is None and self._path is not None:
            if self.kind == "BINTABLE":
                rows = np.fromfile(self._path, dtype=self._dtype, count=self.nrows, offset=self._offset)
                self._data = {}
                for name, letter, repeat in self.columns:
                    col = rows[name]
                    if letter == "A":
                        col = np.asarray([bytes(s).rstrip(b"\0 ").decode("ascii") for s in col], dtype=str)
                    elif letter == "L":
                        col = col.view(np.uint8) == ord("T")
                    else:
                        col = col.astype(col.dtype.base.newbyteorder("="))
                    self._data[name] = col
            elif self.fits_shape:
                n = int(np.prod(self.fits_shape))
                raw = np.fromfile(self._path, dtype=self._dtype, count=n, offset=self._offset)
                self._data = raw.astype(self._dtype.newbyteorder("=")).reshape(self.shape)
        return self._data


def image_cards(data, primary):
    """The mandatory cards of an image (primary or IMAGE extension) holding ``data``."""
    data = None if data is None else np.asarray(data)
    bitpix = 8 if data is None else _IMAGE_BITPIX.get((data.dtype.kind, data.itemsize))
    if bitpix is None:
        raise ValueError(f"FITS: images of {data.dtype} are not supported")
    cards = [("SIMPLE", True, "conforms to FITS standard")] if primary else [("XTENSION", "IMAGE", "Image extension")]
    cards.append(("BITPIX", bitpix, "array data type"))
    shape = () if data is None else data.shape[::-1]
    cards.append(("NAXIS", len(shape), "number of array dimensions"))
    cards += [(f"NAXIS{i + 1}", int(n)) for i, n in enumerate(shape)]
    cards += [("EXTEND", True)] if primary else [("PCOUNT", 0, "number of parameters"), ("GCOUNT", 1, "number of groups")]
    return cards


def image_hdu(data, cards=(), name=None, primary=False):
    """A primary HDU (``primary=True``) or an IMAGE extension from an array in NumPy axis order and extra cards."""
    h = Header(image_cards(data, primary))
    if name is not None:
        h.append("EXTNAME", name, "extension name")
    for c in cards:
        h.append(*c)
    hdu = HDU(h)
    hdu._data = None if data is None else np.asarray(data)
    return hdu


def bintable_hdu(columns, cards=(), name=None):
    """A BINTABLE extension from ``[(name, tform, array), ...]``; ``A`` columns take sequences of str, the numeric
    ones arrays of shape (nrows,) or (nrows, repeat)."""
    nrows = len(columns[0][2]) if columns else 0
    h = Header([("XTENSION", "BINTABLE", "binary table extension"), ("BITPIX", 8, "array data type"),
                ("NAXIS", 2, "number of array dimensions"), ("NAXIS1", 0, "length of dimension 1"),
                ("NAXIS2", nrows, "length of dimension 2"), ("PCOUNT", 0, "number of group parameters"),
                ("GCOUNT", 1, "number of groups"), ("TFIELDS", len(columns), "number of table fields")])
    width, data = 0, {}
    for n, (cname, tform, arr) in enumerate(columns, start=1):
        repeat, letter = _tform(tform, n)
        if len(arr) != nrows:
            raise ValueError(f"FITS: column {cname} has {len(arr)} rows, the table {nrows}")
        if letter == "A":
            arr = np.asarray([str(s) for s in arr], dtype=str)
            if any(len(s) > repeat for s in arr):
                raise ValueError(f"FITS: column {cname} holds strings longer than {repeat} characters")
            width += repeat
        else:
            arr = np.asarray(arr, dtype=bool if letter == "L" else np.dtype(_TFORM[letter]).newbyteorder("="))
            if arr.shape[1:] not in ((), (repeat,)) or (arr.ndim == 1 and repeat != 1):
                raise ValueError(f"FITS: column {cname} of shape {arr.shape} does not match TFORM {tform!r}")
            width += repeat * np.dtype(_TFORM[letter]).itemsize
        h.append(f"TTYPE{n}", cname, f"label for field {n}")
        h.append(f"TFORM{n}", tform, f"data format of field {n}")
        data[cname] = arr
    h.cards[3] = ("NAXIS1", width, "length of dimension 1")
    if name is not None:
        h.append("EXTNAME", name, "extension name")
    for c in cards:
        h.append(*c)
    hdu = HDU(h)
    hdu._data = data
    return hdu


def _data_bytes(hdu):
    data = hdu.data
    if hdu.kind == "BINTABLE":
        rows = np.zeros(hdu.nrows, dtype=hdu._dtype)
        for name, letter, repeat in hdu.columns:
            col = data[name]
            if letter == "A":
                rows[name] = np.asarray([s.encode("ascii") for s in col], dtype=f"S{repeat}") if len(col) else rows[name]
            elif letter == "L":
                rows[name] = np.where(col, ord("T"), ord("F")).astype(np.int8)
            else:
                rows[name] = col
        return rows.tobytes()
    return b"" if data is None else np.ascontiguousarray(data, dtype=hdu._dtype).tobytes()


def write(path, hdus):
    """HDUs (``image_hdu(..., primary=True)`` first, then extensions) -> a FITS file at ``path`` (replaced if present)."""
    if not hdus or hdus[0].kind != "PRIMARY" or any(h.kind == "PRIMARY" for h in hdus[1:]):
        raise ValueError("FITS: a file is one primary HDU followed by extensions")
    units = []  # (everything is formatted before the file is opened: a refused value leaves no partial file behind)
    for hdu in hdus:
        raw = _data_bytes(hdu)
        if len(raw) != hdu.nbytes:
            raise ValueError(f"FITS: HDU {hdu.name}: {len(raw)} data bytes, the header describes {hdu.nbytes}")
        units.append((hdu.header.tobytes(), raw))
    with builtins.open(path, "wb") as f:
        for head, raw in units:
            f.write(head)
            f.write(raw)
            f.write(b"\0" * (_padded(len(raw)) - len(raw)))


class FitsFile:
    """The HDUs of a file, headers parsed; index by position or EXTNAME."""

    def __init__(self, path):
        self.path = os.fspath(path)
        self.hdus = []
        size = os.path.getsize(self.path)
        with builtins.open(self.path, "rb") as f:
            if f.read(len(SIMPLE_CARD)) != SIMPLE_CARD:
                raise ValueError(f"{self.path}: not a FITS file (no 'SIMPLE = T' card first)")
            pos = 0
            while pos < size:
                f.seek(pos)
                raw = b""
                while True:
                    block = f.read(BLOCK)
                    if len(block) < BLOCK:
                        raise ValueError(f"{self.path}: truncated file (header of HDU {len(self.hdus)} ends mid-block)")
                    raw += block
                    if any(raw[i:i + 8] == b"END     " for i in range(len(raw) - BLOCK, len(raw), CARD)):
                        break
                hdu = HDU(Header.parse(raw), self.path, pos + len(raw))
                if (self.hdus == []) != (hdu.kind == "PRIMARY"):
                    raise ValueError(f"{self.path}: HDU {len(self.hdus)} is " + ("not a primary HDU" if not self.hdus else "a second primary HDU"))
                if hdu._offset + hdu.nbytes > size:
                    raise ValueError(f"{self.path}: truncated file (data of HDU {len(self.hdus)} need {hdu.nbytes} bytes, "
                                     f"{size - hdu._offset} are left)")
                self.hdus.append(hdu)
                pos = hdu._offset + _padded(hdu.nbytes)

    def __len__(self):
        return len(self.hdus)

    def __iter__(self):
        return iter(self.hdus)

    def __contains__(self, name):
        return any(h.name == name for h in self.hdus)

    def __getitem__(self, key):
        if isinstance(key, int):
            return self.hdus[key]
        for h in self.hdus:
            if h.name == key:
                return h
        raise KeyError(f"{self.path}: no HDU named {key}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def open(path):  # noqa: A001  (the name hdf5.open uses)
    return FitsFile(path)
