"""What a call enqueues, read from a stream capture: call(stream) runs on a fresh stream captured into a graph, whose kernel
nodes are read (kernel name, grid, block, dynamic LDS) and which is then destroyed -- never instantiated, never launched."""
import ctypes as C
import re


class _Dim3(C.Structure):
    _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint)]


class _KernelNodeParams(C.Structure):  # hipKernelNodeParams (hip_runtime_api.h)
    _fields_ = [("blockDim", _Dim3), ("extra", C.c_void_p), ("func", C.c_void_p), ("gridDim", _Dim3),
                ("kernelParams", C.c_void_p), ("sharedMemBytes", C.c_uint)]


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipKernelNameRefByPtr.restype = C.c_char_p
    hip.hipKernelNameRefByPtr.argtypes = [C.c_void_p, C.c_void_p]
    return hip


def kernels_enqueued(call):
    """(call's return value, [(name or None, grid, block, lds)] of the kernel nodes in enqueue order)"""
    hip = _hip()
    s, g, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    assert hip.hipStreamCreate(C.byref(s)) == 0
    try:
        assert hip.hipStreamBeginCapture(s, 2) == 0  # hipStreamCaptureModeRelaxed
        rc = call(s.value)
        assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
        assert hip.hipGraphGetNodes(g, None, C.byref(n)) == 0
        nodes = (C.c_void_p * max(n.value, 1))()
        assert hip.hipGraphGetNodes(g, nodes, C.byref(n)) == 0
        out = []
        for i in range(n.value):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            if t.value != 0:  # hipGraphNodeTypeKernel
                continue
            p = _KernelNodeParams()
            assert hip.hipGraphKernelNodeGetParams(C.c_void_p(nodes[i]), C.byref(p)) == 0
            name = hip.hipKernelNameRefByPtr(p.func, s) if p.func else None
            out.append((name.decode() if name else None, (p.gridDim.x, p.gridDim.y, p.gridDim.z),
                        (p.blockDim.x, p.blockDim.y, p.blockDim.z), p.sharedMemBytes))
        assert hip.hipGraphDestroy(g) == 0
        return rc, out
    finally:
        hip.hipStreamDestroy(s)


def kernel_count(call):
    """number of kernels call(stream) puts on a fresh stream"""
    rc, k = kernels_enqueued(call)
    return rc, len(k)


_TYPES = {"h": "u8", "t": "u16", "unsigned char": "u8", "unsigned short": "u16"}


def parse_kernel(name):
    """(base name, template arguments) of a kernel symbol, mangled (_ZN12_GLOBAL__N_1<len><name>I..E..) or demangled
    ("void (anonymous namespace)::name<a, b>(...)"); integers and bools as ints, uint8_t / uint16_t as u8 / u16"""
    if name.startswith("_Z"):
        pos, base = (3 if name.startswith("_ZN") else 2), None
        while pos < len(name) and name[pos].isdigit():
            k = re.match(r"\d+", name[pos:]).group()
            base, pos = name[pos + len(k):pos + len(k) + int(k)], pos + len(k) + int(k)
        args = []
        if pos < len(name) and name[pos] == "I":
            pos += 1
            while name[pos] != "E":
                if name[pos] == "L":  # L<type><value>E
                    end = name.index("E", pos)
                    lit = name[pos + 2:end]
                    args.append(-int(lit[1:]) if lit.startswith("n") else int(lit))
                    pos = end + 1
                else:
                    args.append(_TYPES.get(name[pos], name[pos]))
                    pos += 1
        return base, tuple(args)
    m = re.search(r"(\w+)<([^<>]*)>\s*\(", name) or re.search(r"(\w+)\s*\(", name)
    args = []
    for a in (m.group(2).split(",") if m.lastindex == 2 and m.group(2).strip() else []):
        a = a.strip()
        if a in _TYPES:
            args.append(_TYPES[a])
        elif a in ("true", "false"):
            args.append(int(a == "true"))
        else:
            args.append(int(re.sub(r"^\(.*\)|[uUlL]+$", "", a)))
    return m.group(1), tuple(args)
