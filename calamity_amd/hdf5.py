"""The subset of HDF5 that uvh5 files use, read and written in pure Python and NumPy (no h5py, no libhdf5).

Reader: superblock versions 0 and 1; version-1 object headers (continuation blocks included); symbol-table groups
(version-1 group B-tree, local heap, SNOD nodes); dataspace messages 1 and 2; fixed-point, IEEE float, fixed-length
string, compound and enum datatypes; layout message 3 (compact, contiguous, chunked with a version-1 chunk B-tree);
filter pipelines 1 and 2 with LZF (32000), deflate (1) and shuffle (2).  Anything else -- later superblocks, "OHDR"
headers, link-message or dense groups, variable-length types, unknown filters -- raises ``ValueError`` naming it: this
module never guesses.

Writer: the same structures, for a tree of groups and uncompressed contiguous datasets (superblock 0, version-1 object
headers, one SNOD per group).  The files open in the stock HDF5 library.

Type mapping (both directions): compound {r, i} of one float type <-> complex; 8-bit enum {FALSE=0, TRUE=1} <-> bool;
fixed-length string <-> ``bytes`` (numpy "S" arrays).
"""
import builtins
import mmap
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89HDF\r\n\x1a\n"
UNDEF = 0xFFFFFFFFFFFFFFFF
_FREE_NULL = 1  # "no free block" in a local heap, as the HDF5 library encodes it

# object header message types
_NIL, _DATASPACE, _LINK_INFO, _DATATYPE, _FILL_OLD, _FILL, _LINK, _EXTERNAL, _LAYOUT = 0, 1, 2, 3, 4, 5, 6, 7, 8
_FILTERS, _ATTRIBUTE, _CONTINUATION, _SYMBOL_TABLE = 11, 12, 16, 17
_FILTER_DEFLATE, _FILTER_SHUFFLE, _FILTER_LZF = 1, 2, 32000


def lzf_decompress(src, out_size):
    """LZF (liblzf) stream -> bytes of exactly ``out_size``.  ctrl < 32: a literal run of ctrl + 1 bytes; otherwise a
    back-reference of (ctrl >> 5) + 2 bytes (length field 7: plus the next byte) at distance ((ctrl & 31) << 8) + next + 1."""
    src = bytes(src)
    out = bytearray(out_size)
    ip, op, n = 0, 0, len(src)
    while ip < n:
        ctrl = src[ip]
        ip += 1
        if ctrl < 32:
            run = ctrl + 1
            if ip + run > n or op + run > out_size:
                raise ValueError("LZF: literal run past the end of the stream")
            out[op:op + run] = src[ip:ip + run]
            ip += run
            op += run
            continue
        length = ctrl >> 5
        if length == 7:
            if ip >= n:
                raise ValueError("LZF: truncated stream")
            length += src[ip]
            ip += 1
        if ip >= n:
            raise ValueError("LZF: truncated stream")
        ref = op - ((ctrl & 31) << 8) - src[ip] - 1
        ip += 1
        length += 2
        if ref < 0 or op + length > out_size:
            raise ValueError("LZF: back-reference outside the output")
        if op - ref >= length:  # no overlap: one slice copy
            out[op:op + length] = out[ref:ref + length]
        else:  # overlapping: the copy repeats the last (op - ref) bytes
            for k in range(length):
                out[op + k] = out[ref + k]
        op += length
    if op != out_size:
        raise ValueError(f"LZF: stream decodes to {op} bytes, expected {out_size}")
    return bytes(out)


def _unshuffle(buf, itemsize):
    a = np.frombuffer(buf, dtype=np.uint8)
    n = a.size // itemsize
    body = a[: n * itemsize].reshape(itemsize, n).T.reshape(-1)
    return body.tobytes() + a[n * itemsize:].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# reader
# ---------------------------------------------------------------------------------------------------------------------
class _Buf:
    """Little-endian field reader over a bytes object."""

    def __init__(self, data, pos=0):
        self.d, self.p = data, pos

    def u(self, n):
        v = int.from_bytes(self.d[self.p:self.p + n], "little")
        self.p += n
        return v

    def raw(self, n):
        v = self.d[self.p:self.p + n]
        self.p += n
        return v

    def cstr(self):
        end = self.d.find(b"\0", self.p)
        if end < 0:
            raise ValueError("HDF5: unterminated name")
        v = self.d[self.p:end]
        self.p = end + 1
        return v


def _parse_datatype(b):
    """Datatype message -> (numpy dtype, kind) where kind is None, "complex" or "bool" (the conversions applied after
    the raw read)."""
    head = b.u(1)
    cls, version = head & 0x0F, head >> 4
    bits = b.u(3)
    size = b.u(4)
    if cls == 0:  # fixed point
        b.u(4)  # bit offset, precision
        order = ">" if bits & 1 else "<"
        return np.dtype(f"{order}{'i' if bits & 8 else 'u'}{size}"), None
    if cls == 1:  # IEEE float
        b.u(12)
        if bits & 0x40:
            raise ValueError("HDF5: VAX-order floating point is not supported")
        if size not in (2, 4, 8):
            raise ValueError(f"HDF5: {size}-byte floating point is not supported")
        return np.dtype(f"{'>' if bits & 1 else '<'}f{size}"), None
    if cls == 3:  # fixed-length string
        return np.dtype(f"S{size}"), None
    if cls == 6:  # compound
        nmemb = bits & 0xFFFF
        names, formats, offsets = [], [], []
        for _ in range(nmemb):
            start = b.p
            name = b.cstr()
            if version < 3:
                b.p = start + ((b.p - start + 7) // 8) * 8
                off = b.u(4)
            else:
                off = b.u(max(1, (size.bit_length() + 7) // 8))
            if version == 1:
                ndims = b.u(1)
                b.u(3 + 4 + 4)
                b.u(16)
                if ndims:
                    raise ValueError("HDF5: compound members with array dimensions are not supported")
            mt, mkind = _parse_datatype(b)
            if mkind is not None:
                raise ValueError("HDF5: nested complex/enum compound members are not supported")
            names.append(name.decode())
            formats.append(mt)
            offsets.append(off)
        dt = np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": size})
        if (names == ["r", "i"] and formats[0] == formats[1] and formats[0].kind == "f" and offsets == [0, size // 2]
                and formats[0].itemsize in (4, 8) and formats[0].byteorder in "<=|"):
            return dt, "complex"
        return dt, None
    if cls == 8:  # enum
        nmemb = bits & 0xFFFF
        base, _ = _parse_datatype(b)
        names = []
        for _ in range(nmemb):
            start = b.p
            names.append(b.cstr())
            if version < 3:
                b.p = start + ((b.p - start + 7) // 8) * 8
        values = np.frombuffer(b.raw(nmemb * base.itemsize), dtype=base).tolist()
        if base.itemsize == 1 and dict(zip(names, values)) == {b"FALSE": 0, b"TRUE": 1}:
            return base, "bool"
        return base, None
    names = {2: "time", 4: "bitfield", 5: "opaque", 7: "reference", 9: "variable-length", 10: "array"}
    raise ValueError(f"HDF5: datatype class {cls} ({names.get(cls, 'unknown')}) is not supported")


def _parse_dataspace(b):
    version = b.u(1)
    rank = b.u(1)
    b.u(1)  # flags (maximum dimensions, permutation: not needed for a whole-dataset read)
    if version == 1:
        b.u(5)
        kind = 1 if rank else 0
    elif version == 2:
        kind = b.u(1)
    else:
        raise ValueError(f"HDF5: dataspace message version {version} is not supported")
    if kind == 2:
        raise ValueError("HDF5: null dataspaces are not supported")
    dims = tuple(b.u(8) for _ in range(rank))
    return dims


def _parse_filters(b):
    version = b.u(1)
    nfilt = b.u(1)
    if version == 1:
        b.u(6)
    elif version != 2:
        raise ValueError(f"HDF5: filter pipeline message version {version} is not supported")
    out = []
    for _ in range(nfilt):
        fid = b.u(2)
        namelen = b.u(2) if (version == 1 or fid >= 256) else 0
        b.u(2)  # flags
        nvals = b.u(2)
        if namelen:
            b.raw(((namelen + 7) // 8) * 8 if version == 1 else namelen)
        vals = [b.u(4) for _ in range(nvals)]
        if version == 1 and nvals % 2:
            b.u(4)
        if fid not in (_FILTER_DEFLATE, _FILTER_SHUFFLE, _FILTER_LZF):
            raise ValueError(f"HDF5: filter id {fid} is not supported (only deflate 1, shuffle 2 and LZF 32000)")
        out.append((fid, vals))
    return out


class Group:
    """A symbol-table group: ``g[name]`` -> Group or Dataset, ``g["a/b"]`` walks, ``keys()`` in stored (sorted) order."""

    def __init__(self, f, links):
        self._f, self._links = f, links

    def keys(self):
        return list(self._links)

    def __contains__(self, path):
        try:
            self[path]
            return True
        except KeyError:
            return False

    def __iter__(self):
        return iter(self._links)

    def __getitem__(self, path):
        if not isinstance(path, str):
            raise TypeError(f"HDF5: a group is indexed by member name, not {path!r} (ds[()] reads datasets only)")
        node = self
        for part in [p for p in path.split("/") if p]:
            if not isinstance(node, Group) or part not in node._links:
                raise KeyError(path)
            node = node._f._object(node._links[part])
        return node


class Dataset:
    def __init__(self, f, shape, dtype, kind, layout, filters, fill):
        self._f = f
        self.shape, self._dtype, self._kind = shape, dtype, kind
        self._layout, self.filters, self._fill = layout, filters, fill

    @property
    def dtype(self):
        if self._kind == "complex":
            return np.dtype(f"<c{2 * self._dtype.fields['r'][0].itemsize}")
        return np.dtype(bool) if self._kind == "bool" else self._dtype

    @property
    def layout(self):
        return self._layout[0]

    def __getitem__(self, key):
        if key not in ((), Ellipsis):
            raise ValueError("HDF5: partial reads are not supported; read the whole dataset with ds[()]")
        return self.read()

    def _raw_dtype(self):
        return self.dtype if self._kind == "complex" else self._dtype

    def read(self):
        kind = self._layout[0]
        dt = self._raw_dtype()
        count = int(np.prod(self.shape, dtype=np.int64))
        if kind == "compact":
            arr = np.frombuffer(self._layout[1], dtype=dt, count=count).copy()
        elif kind == "contiguous":
            addr, size = self._layout[1], self._layout[2]
            if addr == UNDEF or count == 0:
                arr = np.full(count, self._fill_value(), dtype=dt)
            else:
                if size < count * dt.itemsize:
                    raise ValueError("HDF5: contiguous storage smaller than the dataspace")
                arr = np.fromfile(self._f.path, dtype=dt, count=count, offset=self._f.base + addr)
        else:
            arr = self._read_chunked(dt)
        arr = arr.reshape(self.shape)
        if self._kind == "bool":
            arr = np.asarray(arr != 0)
        return arr

    def _fill_value(self):
        dt = self._raw_dtype()
        if self._fill is None or len(self._fill) != dt.itemsize:
            return np.zeros((), dtype=dt)
        return np.frombuffer(self._fill, dtype=dt)[0]

    def _read_chunked(self, dt):
        btree, cdims = self._layout[1], self._layout[2]
        shape = self.shape
        rank = len(shape)
        if cdims[-1] != self._dtype.itemsize:
            raise ValueError("HDF5: chunk element size does not match the datatype")
        cshape = tuple(cdims[:rank])
        out = np.empty(shape, dtype=dt)
        out[...] = self._fill_value()
        csize = int(np.prod(cshape, dtype=np.int64)) * dt.itemsize
        if btree == UNDEF:
            return out
        with builtins.open(self._f.path, "rb") as fh:
            for nbytes, mask, offs, addr in self._f._chunk_index(fh, btree, rank):
                fh.seek(self._f.base + addr)
                buf = fh.read(nbytes)
                for n, (fid, vals) in reversed(list(enumerate(self.filters))):
                    if mask & (1 << n):
                        continue  # filter skipped for this chunk
                    if fid == _FILTER_LZF:
                        buf = lzf_decompress(buf, csize)
                    elif fid == _FILTER_DEFLATE:
                        buf = zlib.decompress(buf)
                    elif fid == _FILTER_SHUFFLE:
                        buf = _unshuffle(buf, dt.itemsize)
                if len(buf) != csize:
                    raise ValueError(f"HDF5: chunk at {addr} holds {len(buf)} bytes, expected {csize}")
                chunk = np.frombuffer(buf, dtype=dt).reshape(cshape)
                if any(o % c for o, c in zip(offs, cshape)):
                    raise ValueError("HDF5: chunk offset not on the chunk grid")
                dst = tuple(slice(o, min(o + c, s)) for o, c, s in zip(offs, cshape, shape))
                src = tuple(slice(0, d.stop - d.start) for d in dst)
                if all(d.stop > d.start for d in dst):
                    out[dst] = chunk[src]
        return out


class File(Group):
    """An HDF5 file opened for reading (see the module docstring for the subset)."""

    def __init__(self, path):
        """Opening maps the file (no read of its bulk): the superblock, headers, heaps and B-trees are parsed from the
        mapping on demand; dataset contents are read by ``Dataset.read`` (``np.fromfile`` for contiguous data)."""
        self.path = os.fspath(path)
        with builtins.open(self.path, "rb") as fh:
            if os.fstat(fh.fileno()).st_size < 8:
                raise ValueError(f"{self.path}: no HDF5 signature")
            data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        self._data = data
        sb = -1
        for off in [0] + [512 << k for k in range(20)]:
            if off + 8 > len(data):
                break
            if data[off:off + 8] == SIGNATURE:
                sb = off
                break
        if sb < 0:
            raise ValueError(f"{self.path}: no HDF5 signature")
        b = _Buf(data, sb + 8)
        version = b.u(1)
        if version not in (0, 1):
            raise ValueError(f"{self.path}: HDF5 superblock version {version} is not supported (only 0 and 1)")
        b.u(3)  # free space, root group symbol table, reserved
        b.u(1)  # shared header message format version
        so, sl = b.u(1), b.u(1)
        if (so, sl) != (8, 8):
            raise ValueError(f"{self.path}: HDF5 offsets/lengths of {so}/{sl} bytes are not supported (only 8/8)")
        b.u(1)
        b.u(4)  # group leaf / internal node K
        b.u(4)  # consistency flags
        if version == 1:
            b.u(4)
        self.base = b.u(8)
        b.u(8)  # free space info
        b.u(8)  # end of file
        b.u(8)  # driver info
        b.u(8)  # root: link name offset
        root = b.u(8)
        self._cache = {}
        g = self._object(root)
        if not isinstance(g, Group):
            raise ValueError(f"{self.path}: the root object is not a group")
        super().__init__(self, g._links)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Release the mapping (datasets of a closed file can no longer be read)."""
        self._data.close()

    def _at(self, addr, n):
        a = self.base + addr
        if addr == UNDEF or a + n > len(self._data):
            raise ValueError(f"{self.path}: structure at {addr} lies outside the file")
        return self._data[a:a + n]

    def _messages(self, addr):
        if self._at(addr, 4) == b"OHDR":
            raise ValueError(f"{self.path}: version-2 object headers (OHDR) are not supported")
        b = _Buf(self._data, self.base + addr)
        version = b.u(1)
        if version != 1:
            raise ValueError(f"{self.path}: object header version {version} is not supported")
        b.u(1)
        nmsg = b.u(2)
        b.u(4)
        size = b.u(4)
        blocks = [(self.base + addr + 16, size)]
        msgs = []
        while blocks and len(msgs) < nmsg:
            start, size = blocks.pop(0)
            p = start
            while p + 8 <= start + size and len(msgs) < nmsg:
                mb = _Buf(self._data, p)
                mtype, msize, mflags = mb.u(2), mb.u(2), mb.u(1)
                body = self._data[p + 8:p + 8 + msize]
                p += 8 + msize
                if mtype == _CONTINUATION:
                    cb = _Buf(body)
                    blocks.append((self.base + cb.u(8), cb.u(8)))
                msgs.append((mtype, mflags, body))
        return msgs

    def _object(self, addr):
        if addr in self._cache:
            return self._cache[addr]
        msgs = self._messages(addr)
        types = {m[0] for m in msgs}
        if _SYMBOL_TABLE in types:
            body = next(m[2] for m in msgs if m[0] == _SYMBOL_TABLE)
            b = _Buf(body)
            obj = Group(self, self._group_links(b.u(8), b.u(8)))
        elif _LINK in types or _LINK_INFO in types:
            raise ValueError(f"{self.path}: link-message (compact or dense) groups are not supported")
        elif _DATASPACE in types and _DATATYPE in types and _LAYOUT in types:
            obj = self._dataset(msgs)
        else:
            raise ValueError(f"{self.path}: object at {addr} is neither a symbol-table group nor a dataset")
        self._cache[addr] = obj
        return obj

    def _dataset(self, msgs):
        shape = dtype = kind = layout = fill = None
        filters = []
        for mtype, mflags, body in msgs:
            if mtype in (_DATATYPE, _DATASPACE, _FILL, _FILL_OLD, _LAYOUT, _FILTERS) and mflags & 2:
                raise ValueError(f"{self.path}: shared (committed) header messages are not supported")
            b = _Buf(body)
            if mtype == _DATASPACE:
                shape = _parse_dataspace(b)
            elif mtype == _DATATYPE:
                dtype, kind = _parse_datatype(b)
            elif mtype == _FILTERS:
                filters = _parse_filters(b)
            elif mtype == _FILL:
                version = b.u(1)
                if version in (1, 2):
                    b.u(2)  # allocation time, write time
                    if b.u(1) or version == 1:
                        n = b.u(4)
                        fill = b.raw(n) if n else None
                elif version == 3:
                    flags = b.u(1)
                    if flags & 0x20:
                        n = b.u(4)
                        fill = b.raw(n)
                else:
                    raise ValueError(f"{self.path}: fill value message version {version} is not supported")
            elif mtype == _FILL_OLD and fill is None:
                n = b.u(4)
                fill = b.raw(n) if n else None
            elif mtype == _LAYOUT:
                version = b.u(1)
                if version != 3:
                    raise ValueError(f"{self.path}: data layout message version {version} is not supported (only 3)")
                cls = b.u(1)
                if cls == 0:
                    n = b.u(2)
                    layout = ("compact", b.raw(n))
                elif cls == 1:
                    layout = ("contiguous", b.u(8), b.u(8))
                elif cls == 2:
                    nd = b.u(1)
                    addr = b.u(8)
                    layout = ("chunked", addr, tuple(b.u(4) for _ in range(nd)))
                else:
                    raise ValueError(f"{self.path}: data layout class {cls} is not supported")
            elif mtype == _EXTERNAL:
                raise ValueError(f"{self.path}: external data files are not supported")
            elif mtype > 0x18 and mflags & 0x80:
                raise ValueError(f"{self.path}: unknown header message type {mtype} is marked as required")
        if layout[0] != "chunked" and filters:
            raise ValueError(f"{self.path}: filters on non-chunked storage")
        return Dataset(self, shape, dtype, kind, layout, filters, fill)

    def _group_links(self, btree, heap):
        h = _Buf(self._at(heap, 32))
        if h.raw(4) != b"HEAP":
            raise ValueError(f"{self.path}: bad local heap signature at {heap}")
        h.u(4)
        hsize = h.u(8)
        h.u(8)
        names = self._at(h.u(8), hsize)
        links = {}
        for snod in self._btree_children(btree, 0, 8):
            s = _Buf(self._at(snod, 8))
            if s.raw(4) != b"SNOD":
                raise ValueError(f"{self.path}: bad symbol table node signature at {snod}")
            s.u(2)
            n = s.u(2)
            e = _Buf(self._at(snod + 8, 40 * n))
            for _ in range(n):
                name_off, obj = e.u(8), e.u(8)
                e.raw(24)
                end = names.index(b"\0", name_off)
                links[names[name_off:end].decode()] = obj
        return links

    def _btree_children(self, addr, node_type, key_size):
        return [child for _, child in self._btree_entries(addr, node_type, key_size)]

    def _btree_entries(self, addr, node_type, key_size):
        """(left key, child address) of every leaf entry of a version-1 B-tree, left to right."""
        b = _Buf(self._at(addr, 24))
        if b.raw(4) != b"TREE":
            raise ValueError(f"{self.path}: bad B-tree signature at {addr}")
        t, level, n = b.u(1), b.u(1), b.u(2)
        if t != node_type:
            raise ValueError(f"{self.path}: B-tree at {addr} has node type {t}, expected {node_type}")
        e = _Buf(self._at(addr + 24, n * (key_size + 8) + key_size))
        entries = []
        for _ in range(n):
            key = e.raw(key_size)
            child = e.u(8)
            if level > 0:
                entries.extend(self._btree_entries(child, node_type, key_size))
            else:
                entries.append((key, child))
        return entries

    def _chunk_index(self, fh, btree, rank):
        """(stored size, filter mask, element offsets, address) of every allocated chunk."""
        key_size = 8 + 8 * (rank + 1)
        out = []
        for key, child in self._btree_entries(btree, 1, key_size):
            k = _Buf(key)
            nbytes, mask = k.u(4), k.u(4)
            offs = tuple(k.u(8) for _ in range(rank))
            out.append((nbytes, mask, offs, child))
        return out


def open(path):  # noqa: A001 (the module's public name, as in h5py.File)
    return File(path)


# ---------------------------------------------------------------------------------------------------------------------
# writer
# ---------------------------------------------------------------------------------------------------------------------
def _pad8(b):
    return b + b"\0" * (-len(b) % 8)


def _datatype_message(dt):
    """numpy dtype (bool / complex / int / float / S) -> HDF5 datatype message bytes (version 1 encodings)."""
    dt = np.dtype(dt)
    if dt.kind == "b":
        base = _datatype_message(np.dtype("i1"))
        names = _pad8(b"FALSE\0") + _pad8(b"TRUE\0")
        return struct.pack("<B3sI", 0x18, (2).to_bytes(3, "little"), 1) + base + names + b"\x00\x01"
    if dt.kind == "c":
        half = np.dtype(f"<f{dt.itemsize // 2}")
        body = b""
        for name, off in ((b"r", 0), (b"i", half.itemsize)):
            body += _pad8(name + b"\0") + struct.pack("<IB3sI4s16s", off, 0, b"", 0, b"", b"") + _datatype_message(half)
        return struct.pack("<B3sI", 0x16, (2).to_bytes(3, "little"), dt.itemsize) + body
    if dt.kind in "iu":
        bits = (8 if dt.kind == "i" else 0) | (1 if dt.byteorder == ">" else 0)
        return struct.pack("<B3sIHH", 0x10, bits.to_bytes(3, "little"), dt.itemsize, 0, 8 * dt.itemsize)
    if dt.kind == "f":
        if dt.itemsize == 8:
            bits, props = 0x3F20, (0, 64, 52, 11, 0, 52, 1023)
        elif dt.itemsize == 4:
            bits, props = 0x1F20, (0, 32, 23, 8, 0, 23, 127)
        else:
            raise ValueError(f"HDF5 writer: float{8 * dt.itemsize} is not supported")
        bits |= 1 if dt.byteorder == ">" else 0
        return struct.pack("<B3sIHHBBBBI", 0x11, bits.to_bytes(3, "little"), dt.itemsize, *props)
    if dt.kind == "S":
        return struct.pack("<B3sI", 0x13, (1).to_bytes(3, "little"), max(1, dt.itemsize))  # null-padded ASCII
    raise ValueError(f"HDF5 writer: numpy dtype {dt} is not supported")


def _message(mtype, body, flags=0):
    body = _pad8(body)
    return struct.pack("<HHB3s", mtype, len(body), flags, b"") + body


def _object_header(messages):
    body = b"".join(messages)
    return struct.pack("<BBHII4s", 1, 0, len(messages), 1, len(body), b"") + body


class _Writer:
    def __init__(self, fh):
        self.fh = fh
        self.pos = fh.tell()

    def put(self, data):
        """Append 8-byte-aligned bytes (or an array's buffer), return the address."""
        pad = -self.pos % 8
        if pad:
            self.fh.write(b"\0" * pad)
            self.pos += pad
        addr = self.pos
        if isinstance(data, np.ndarray):
            data.tofile(self.fh) if data.flags.c_contiguous else self.fh.write(data.tobytes())
            self.pos += data.nbytes
        else:
            self.fh.write(data)
            self.pos += len(data)
        return addr


def _as_dataset_array(v):
    if isinstance(v, (bytes, str)):
        v = v.encode() if isinstance(v, str) else v
        return np.array(v, dtype=f"S{max(1, len(v))}")
    a = np.asarray(v)
    if a.dtype.kind == "U":
        a = np.char.encode(a, "ascii")
    if a.dtype.kind == "S" and a.dtype.itemsize == 0:
        a = a.astype("S1")
    if a.dtype.kind in "iufc" and a.dtype.byteorder == ">":
        a = a.astype(a.dtype.newbyteorder("<"))
    return a


def _write_dataset(w, arr):
    arr = _as_dataset_array(arr)
    arr = arr if arr.flags.c_contiguous else arr.copy()  # (not ascontiguousarray: that makes scalars 1-D)
    if arr.dtype.kind == "b":
        raw = arr.view(np.int8)
    elif arr.dtype.kind == "c":
        raw = arr.astype(arr.dtype.newbyteorder("<"), copy=False)
    else:
        raw = arr
    addr = w.put(raw) if arr.size else UNDEF
    space = struct.pack("<BBB5s", 1, arr.ndim, 0, b"") + b"".join(struct.pack("<Q", d) for d in arr.shape)
    fill = struct.pack("<BBBB", 2, 2, 2, 0)  # version 2, allocation late, written if set, no fill value defined
    layout = struct.pack("<BBQQ", 3, 1, addr, arr.nbytes)
    msgs = [_message(_DATASPACE, space), _message(_DATATYPE, _datatype_message(arr.dtype), flags=1),
            _message(_FILL, fill, flags=1), _message(_LAYOUT, layout)]
    return w.put(_object_header(msgs))


def _write_group(w, tree, leaf_k, internal_k):
    """Children first (their addresses go into the symbol table), then heap, SNOD, B-tree and the group's header."""
    names = sorted(tree, key=lambda s: s.encode())
    entries = []
    for name in names:
        v = tree[name]
        if isinstance(v, dict):
            addr, scratch = _write_group(w, v, leaf_k, internal_k)
            entries.append((name, addr, 1, scratch))
        else:
            entries.append((name, _write_dataset(w, v), 0, b""))
    heap_data, offsets = bytearray(b"\0" * 8), []
    for name in names:
        offsets.append(len(heap_data))
        heap_data += _pad8(name.encode() + b"\0")
    heap_data += b"\0" * 8 if len(heap_data) == 8 else b""
    data_addr = w.put(bytes(heap_data))
    heap = w.put(b"HEAP" + struct.pack("<B3sQQQ", 0, b"", len(heap_data), _FREE_NULL, data_addr))
    snod = b"SNOD" + struct.pack("<BBH", 1, 0, len(entries))
    for (name, addr, cache, scratch), off in zip(entries, offsets):
        snod += struct.pack("<QQI4s16s", off, addr, cache, b"", scratch)
    snod += b"\0" * (8 + 2 * leaf_k * 40 - len(snod))
    snod_addr = w.put(snod)
    last_key = offsets[-1] if offsets else 0
    tree_node = b"TREE" + struct.pack("<BBHQQ", 0, 0, 1, UNDEF, UNDEF) + struct.pack("<QQQ", 0, snod_addr, last_key)
    tree_node += b"\0" * (24 + (2 * internal_k + 1) * 8 + 2 * internal_k * 8 - len(tree_node))
    btree = w.put(tree_node)
    header = w.put(_object_header([_message(_SYMBOL_TABLE, struct.pack("<QQ", btree, heap))]))
    return header, struct.pack("<QQ", btree, heap)


def _max_group_size(tree):
    sub = [_max_group_size(v) for v in tree.values() if isinstance(v, dict)]
    return max([len(tree)] + sub)


def write(path, tree):
    """Write ``tree`` -- a dict of name -> dict (a group) or array-like (a dataset: numeric, bool, complex, bytes / "S"
    arrays; ``str`` values are stored as fixed-length ASCII) -- as an HDF5 file in the subset this module reads."""
    leaf_k = max(4, (_max_group_size(tree) + 1) // 2)  # every group fits one symbol table node
    internal_k = 16
    with builtins.open(os.fspath(path), "wb") as fh:
        fh.write(b"\0" * 96)
        w = _Writer(fh)
        root, scratch = _write_group(w, tree, leaf_k, internal_k)
        eof = w.pos
        sb = SIGNATURE + struct.pack("<BBBBBBBBHHI", 0, 0, 0, 0, 0, 8, 8, 0, leaf_k, internal_k, 0)
        sb += struct.pack("<QQQQ", 0, UNDEF, eof, UNDEF)
        sb += struct.pack("<QQI4s16s", 0, root, 1, b"", scratch)
        fh.seek(0)
        fh.write(sb)

