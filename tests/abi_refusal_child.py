"""The child process of tests/test_abi_refusals.py: makes a list of C ABI calls with NO device and reports their return codes.

Run as `python abi_refusal_child.py` with {"lib": path, "calls": [...]} as JSON on stdin.  The first act is to ask the HIP runtime
that libecm_hip.so links for the device count; if a device is visible, no ABI call is made at all.  Output, one line each:
    DEVICES <n>          the count the runtime reported (0 also when it answered hipErrorNoDevice), or `unknown: why`, which the
                         parent takes as a failure, not as a reason to skip
    R <id> <code>        the return value of call <id>, written as soon as the call is back (a crash names the call after the last)
    DONE

A call is {"id": str, "fn": name, "res": "i" | "q", "args": [arg, ...]}, an arg one of
    {"t": "i" | "q" | "f", "v": number}                     int / long long / float by value
    {"t": "q", "ref": id, "add": k}                         long long: the result of the earlier call `id`, plus k
    {"t": "p", "v": "dev" | None, "off": k}                 a device pointer: an address k bytes into one live zero-filled host
                                                            buffer (never dereferenced: no kernel runs; the offsets keep the
                                                            operands of a call apart for the entries that refuse aliases), or NULL
    {"t": "p", "host": "i" | "f" | "d", "vals": [...]}      a HOST array the entry itself reads
    {"t": "p", "ptrs": n}                                   a HOST array of n device pointers
execute() is also what the planted-defect test runs in-process, against ctypes callbacks."""
import ctypes as C
import json
import re
import sys

SCALAR = {"i": C.c_int, "q": C.c_longlong, "f": C.c_float}
HOST = {"i": C.c_int, "f": C.c_float, "d": C.c_double}
DEV_BYTES = 16384
HIP_ERROR_NO_DEVICE = 100


def execute(calls, resolve, report=lambda cid, rc: None):
    """Run `calls` in order through resolve(name) -> callable taking ctypes values; {id: return value}."""
    dev = (C.c_char * (DEV_BYTES + 256))()                  # zero-filled, alive for the whole run
    dev_addr = (C.addressof(dev) + 255) & ~255              # aligned as device allocations are
    keep, out = [], {}
    for call in calls:
        argv = []
        for a in call["args"]:
            if a["t"] != "p":
                v = out[a["ref"]] + a.get("add", 0) if "ref" in a else a["v"]
                argv.append(SCALAR[a["t"]](v))
            elif "host" in a:
                arr = (HOST[a["host"]] * len(a["vals"]))(*a["vals"])
                keep.append(arr)
                argv.append(C.c_void_p(C.addressof(arr)))
            elif "ptrs" in a:
                arr = (C.c_void_p * a["ptrs"])(*[dev_addr + DEV_BYTES // 2] * a["ptrs"])
                keep.append(arr)
                argv.append(C.c_void_p(C.addressof(arr)))
            else:
                argv.append(C.c_void_p(dev_addr + a.get("off", 0) if a["v"] == "dev" else None))
        out[call["id"]] = int(resolve(call["fn"], call["res"], [type(v) for v in argv])(*argv))
        report(call["id"], out[call["id"]])
    return out


def visible_devices(lib_path):
    """The device count of the libamdhip64 that the loaded libecm_hip.so links (found in this process's map, not by name)."""
    C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    with open("/proc/self/maps") as f:
        paths = sorted(set(re.findall(r"(/\S*libamdhip64\.so[\w.]*)", f.read())))
    if not paths:
        return "unknown: no libamdhip64 in the process map"
    n = C.c_int(-1)
    rc = C.CDLL(paths[0]).hipGetDeviceCount(C.byref(n))
    if rc == HIP_ERROR_NO_DEVICE:
        return 0
    return n.value if rc == 0 and n.value >= 0 else f"unknown: hipGetDeviceCount returned {rc}, count {n.value}"


def main():
    job = json.load(sys.stdin)
    n = visible_devices(job["lib"])
    print("DEVICES", n, flush=True)
    if n != 0:
        return 0
    lib = C.CDLL(job["lib"])

    def resolve(name, res, argtypes):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SCALAR[res], argtypes
        return fn

    execute(job["calls"], resolve, lambda cid, rc: print("R", cid, rc, flush=True))
    print("DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
