"""The "KnnOperator" of the host mirror, driven by the reference's OWN Python layer (Graph.search, KnnOption,
IndexOption, set_knn_metric) on this engine's pywrap_graphlearn, against the contract's restatement; and the host
request classes' unit test.  The script is tests/scripts/refpy_knn_search.py."""
import os
import subprocess
import sys

import pytest

import refpy

LIB = os.path.join(refpy.ROOT, "graph-learn_amd", "lib")


@pytest.mark.gpu
@pytest.mark.skipif(not refpy.staged(), reason="reference python layer not staged (scripts/stage_refpy.py)")
def test_reference_graph_search_runs_on_the_device_table(tmp_path):
    script = os.path.join(refpy.ROOT, "tests", "scripts", "refpy_knn_search.py")
    out = subprocess.run([sys.executable, script, str(tmp_path)], env=refpy.env(), cwd=str(tmp_path),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "KNN OK" in out.stdout, out.stdout[-4000:]


def test_knn_request_unittest_on_cpu():
    """KnnRequest fields, Partition to every shard, Stitch under the total order: host code, no device"""
    r = subprocess.run([os.path.join(LIB, "knn_request_unittest")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout
