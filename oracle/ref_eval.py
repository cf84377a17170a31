"""The reference's mesh evaluation, built and imported for the generator of tests/golden/eval_ref.npz (TEST
INFRASTRUCTURE; the authoring container only -- no test and nothing on the GPU box reads the reference).

    from oracle import ref_eval
    R = ref_eval.load()          # R.check_mesh_contains, R.implicit_waterproofing, R.eval_pointcloud, R.Mesh

What it does, in order:
  * evaluation/libmesh/triangle_hash.pyx is turned into C++ by the installed Cython and compiled against the Python and
    numpy headers into oracle/_ref/ (ignored by git: neither the generated C++ nor the extension is ever committed);
  * the extension is registered under the name the reference imports it by (evaluation.libmesh.triangle_hash), and the
    reference's inside_mesh.py, implicit_waterproofing.py and eval_util.py are imported from the reference tree itself,
    never copied (bytecode writing is off);
  * trimesh is absent here and the three files only import it, so the name is an empty stub.  `Mesh` below stands in for
    the trimesh.Trimesh the reference is handed: `vertices` (float64), `faces`, `copy()` and `apply_transform(m)`.
    ASSUMPTION: apply_transform is np.dot(m[:3, :3], v.T).T -- the same expression implicit_waterproofing.py:44 applies
    to the query points, with the zero translation the reference pads in dropped.  trimesh's own arithmetic (a
    homogeneous 4x4 product) has not been run here.

implicit_waterproofing.py calls check_mesh_contains at its default hash_resolution (512).  `implicit_waterproofing(mesh,
points, res)` below runs the reference's function with that one name bound to the same function at `res`, so the retries
can be recorded at other resolutions; nothing else of the reference is touched.
"""
import functools
import importlib
import importlib.util
import os
import subprocess
import sys
import sysconfig
import types

import numpy as np

from .gen_golden import REF

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
_EXT_NAME = "evaluation.libmesh.triangle_hash"


class Mesh:
    """The stand-in for trimesh.Trimesh (see the module docstring for the assumption in apply_transform)."""

    def __init__(self, vertices, faces):
        self.vertices = np.array(vertices, dtype=np.float64)
        self.faces = np.array(faces, dtype=np.int64)

    def copy(self):
        return Mesh(self.vertices, self.faces)

    def apply_transform(self, m):
        m = np.asarray(m, dtype=np.float64)
        self.vertices = np.dot(m[:3, :3], self.vertices.T).T
        return self


def build_extension(ref=None, force=False):
    """triangle_hash.pyx -> oracle/_ref/triangle_hash<EXT_SUFFIX>; returns the extension's path."""
    ref = ref or os.environ.get("LIST_REFERENCE", REF)
    pyx = os.path.join(ref, "evaluation", "libmesh", "triangle_hash.pyx")
    os.makedirs(OUT, exist_ok=True)
    cpp = os.path.join(OUT, "triangle_hash.cpp")
    ext = os.path.join(OUT, "triangle_hash" + sysconfig.get_config_var("EXT_SUFFIX"))
    if not force and os.path.exists(ext) and os.path.getmtime(ext) >= os.path.getmtime(pyx):
        return ext
    subprocess.run([sys.executable, "-m", "cython", "--cplus", "-3", "-o", cpp, pyx], check=True)
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-shared", "-fPIC", "-std=c++17", "-w",
                    "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION",
                    "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(), cpp, "-o", ext], check=True)
    return ext


@functools.lru_cache(maxsize=None)
def load(ref=None):
    """Build (if needed) and import: a namespace with the reference's functions and the stand-in Mesh."""
    ref = ref or os.environ.get("LIST_REFERENCE", REF)
    ext = build_extension(ref)
    sys.dont_write_bytecode = True
    if ref not in sys.path:
        sys.path.insert(0, ref)
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    if _EXT_NAME not in sys.modules:
        spec = importlib.util.spec_from_file_location(_EXT_NAME, ext)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules[_EXT_NAME] = mod
    inside = importlib.import_module("evaluation.libmesh.inside_mesh")          # reference
    iw = importlib.import_module("evaluation.implicit_waterproofing")           # reference
    eu = importlib.import_module("evaluation.eval_util")                        # reference
    for m in (inside, iw, eu):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref) + os.sep), m.__file__

    def implicit_waterproofing(mesh, points, res=512):
        orig = iw.check_mesh_contains
        iw.check_mesh_contains = lambda m, p: inside.check_mesh_contains(m, p, res)
        try:
            return iw.implicit_waterproofing(mesh, points)
        finally:
            iw.check_mesh_contains = orig

    return types.SimpleNamespace(Mesh=Mesh, check_mesh_contains=inside.check_mesh_contains,
                                 implicit_waterproofing=implicit_waterproofing, eval_pointcloud=eu.eval_pointcloud,
                                 to_rotation_matrix=iw.to_rotation_matrix)


if __name__ == "__main__":
    print(build_extension(force="--force" in sys.argv))
