"""The one builder of the stand-alone CPU programs tests/*_emulate.cpp: each has its own main() and runs as a child process of the test
that drives it (the drivers are the build_emulator functions of the *_cases.py modules and the fixtures of the *_host test files)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compiler():
    """The host C++ compiler: $CXX, then c++, g++, clang++ on the path, then ROCm's clang."""
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    return cxx


def build(name, d, sanitize=False):
    """tests/`name`.cpp -> `d`/`name`, returned as a string.  sanitize=True builds under the sanitizers where the compiler can link and run
    an empty program under them, and plain, saying so, where it cannot."""
    cxx, exe = compiler(), str(d / name)
    if sanitize:
        probe = str(d / "probe.cpp")
        open(probe, "w").write("int main() { return 0; }\n")
        if subprocess.call([cxx] + SANITIZE + ["-o", str(d / "probe"), probe], stderr=subprocess.DEVNULL) != 0 or subprocess.call([str(d / "probe")]) != 0:
            sanitize = False
            print(f"{name}: the host compiler cannot link -fsanitize=address,undefined; built plain")
    mode = ["-O1", "-g"] + SANITIZE if sanitize else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off"] + mode + ["-o", exe, os.path.join(HERE, name + ".cpp")], timeout=300)
    return exe
