"""What the tests that run several ranks as several PROCESSES share: the launchers of the gloo and the ipc-pull workers, the probe for
peer-memory reads, and the lists of schedule configurations."""
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(nranks, case, configs, timeout=300):
    port = free_port()
    procs = []
    for r in range(nranks):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(nranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gloo_worker.py"), case, configs],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return procs, outs


def launch_ipc(nranks, case, configs, backend="oracle", timeout=600, extra_env=None):
    session = "t%d_%x" % (os.getpid(), time.time_ns())
    with tempfile.TemporaryDirectory(prefix="hnh_ipc_") as outdir:
        procs = []
        for r in range(nranks):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(nranks), OMP_NUM_THREADS="2", HNH_TEST_BACKEND=backend, HNH_IPC_WAIT_S="120",
                       HSA_ENABLE_IPC_MODE_LEGACY="0")
            env.update(extra_env or {})
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ipc_worker.py"), session, outdir, case, configs], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = []
        try:
            for p in procs:
                outs.append(p.communicate(timeout=timeout)[0])
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
    return procs, outs


def can_read_peer_memory():
    """The test double's pull is process_vm_readv: needs ptrace permission between the test's own processes."""
    import ctypes
    libc = ctypes.CDLL(None, use_errno=True)
    r, w = os.pipe()
    buf = ctypes.create_string_buffer(b"x" * 8, 8)
    pid = os.fork()
    if pid == 0:
        os.read(r, 1)
        os._exit(0)

    class IoVec(ctypes.Structure):
        _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_size_t)]
    out = ctypes.create_string_buffer(8)
    loc, rem = IoVec(ctypes.addressof(out), 8), IoVec(ctypes.addressof(buf), 8)
    got = libc.process_vm_readv(pid, ctypes.byref(loc), 1, ctypes.byref(rem), 1, 0)
    os.write(w, b"x")
    os.waitpid(pid, 0)
    return got == 8


ALL_2 = ("15d_fusion1:1:mesh:4;15d_fusion2:1:mesh:4;15d_fusion2:1:mesh:2;15d_fusion2:1:relay:1;15d_fusion2:2:mesh:4;15d_sparse:1:mesh:4;"
         "15d_sparse:2:mesh:4;25d_dense_replicate:2:mesh:4;25d_sparse_replicate:2:mesh:4;als@15d_fusion2:1:mesh:4;als@15d_sparse:1:mesh:4")
ALL_4 = ("15d_fusion2:1:mesh:4;15d_fusion2:1:relay:1;15d_fusion2:2:mesh:2;15d_fusion1:2:mesh:4;15d_sparse:1:mesh:4;25d_dense_replicate:1:mesh:4;"
         "25d_sparse_replicate:1:mesh:4;als@15d_fusion2:1:mesh:4;als@25d_dense_replicate:1:mesh:4")
ALL_8 = ("15d_fusion2:1:mesh:4;15d_fusion2:1:mesh:8;15d_fusion2:1:relay:1;15d_fusion2:2:mesh:4;15d_fusion2:4:mesh:2;15d_fusion1:1:mesh:4;"
         "15d_sparse:2:mesh:4;25d_dense_replicate:2:mesh:4;25d_sparse_replicate:2:mesh:4;als@15d_fusion2:1:mesh:4")
