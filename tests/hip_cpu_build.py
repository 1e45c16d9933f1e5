"""The g++ line of the programs that run a kernel file's own text on the CPU (tests/c/*_kernel_main.cpp): ASan + UBSan,
tests/c/hip_cpu in front of the HIP and rocPRIM headers, the kernel files on the include path."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(main, exe, *flags):
    """tests/c/<main> -> exe.  flags: -DHIP_CPU_SERIAL for a kernel file without barrier, LDS or wave operation."""
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", "-I", os.path.join(ROOT, "tests", "c", "hip_cpu"),
                           "-I", os.path.join(ROOT, "gnuais_amd", "csrc"), *flags, os.path.join(ROOT, "tests", "c", main),
                           "-o", str(exe)])
    return str(exe)
