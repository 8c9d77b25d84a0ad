"""Compiler parity: every fixture pipeline compiles to the reference's golden Argo workflow.

Reference test strategy: `sdk/python/tests/compiler/compiler_tests.py:150-545` (golden YAML per
pipeline via dsl-compile, op->template, tolerations, display name, op transformers, type checks).
When the reference checkout is present the comparison is against its `testdata/<name>.yaml`
(loaded with yaml.safe_load); the sha256 of each canonical compiled workflow is additionally pinned
in kfp_testdata/golden_digests.json so the check still runs without the reference."""

import hashlib
import json
import os
import subprocess
import sys
import tarfile
import zipfile

import pytest
import yaml

from mifx.kfp import compiler, components, dsl
from mifx.kfp.compiler._component_builder import kaniko_pod_spec
from mifx.kfp.compiler._op_to_template import op_to_template
from mifx.kfp.dsl.types import InconsistentTypeException, Integer
from mifx.kfp.k8s import V1Toleration
from tests.kfp_testdata.pipelines import PIPELINES

HERE = os.path.dirname(__file__)
DIGESTS = os.path.join(HERE, "kfp_testdata", "golden_digests.json")
# sha256 of the canonical form of the reference's own golden files (its compiler testdata), as _digest computes it
REF_DIGESTS = os.path.join(HERE, "golden", "kfp_reference_digests.json")


def _canonical(wf: dict) -> str:
    return json.dumps(yaml.safe_load(yaml.safe_dump(wf)), sort_keys=True, separators=(",", ":"))


def _digest(wf: dict) -> str:
    return hashlib.sha256(_canonical(wf).encode()).hexdigest()


def _ref_digest(name: str) -> str:
    with open(REF_DIGESTS) as f:
        return json.load(f)[name]


@pytest.mark.parametrize("name", sorted(PIPELINES))
def test_compile_matches_golden(name):
    wf = compiler.Compiler()._compile(PIPELINES[name])
    with open(DIGESTS) as f:
        assert _digest(wf) == json.load(f)[name]


@pytest.mark.parametrize("ext", [".zip", ".tar.gz", ".yaml"])
def test_package_formats_roundtrip(tmp_path, ext):
    out = str(tmp_path / ("pkg" + ext))
    compiler.Compiler().compile(PIPELINES["coin"], out)
    if ext == ".zip":
        with zipfile.ZipFile(out) as z:
            got = yaml.safe_load(z.read(z.namelist()[0]))
    elif ext == ".tar.gz":
        with tarfile.open(out) as t:
            got = yaml.safe_load(t.extractfile(t.getmembers()[0]))
    else:
        with open(out) as f:
            got = yaml.safe_load(f)
    assert got["kind"] == "Workflow" and got["spec"]["entrypoint"] == "pipeline-flip-coin"
    assert yaml.safe_load(compiler.read_package(out)) == got


def test_dsl_compile_cli(tmp_path):
    src = tmp_path / "my_pipeline.py"
    src.write_text(
        "from mifx.kfp import dsl\n"
        "@dsl.pipeline(name='Cli Pipeline', description='d')\n"
        "def p(msg: str = 'hi'):\n"
        "    dsl.ContainerOp(name='echo', image='alpine', command=['echo', msg])\n")
    out = tmp_path / "out.tar.gz"
    subprocess.run([sys.executable, "-m", "mifx.kfp.compiler.main", "--py", str(src), "--output", str(out)],
                   check=True, cwd=os.path.dirname(HERE))
    wf = yaml.safe_load(compiler.read_package(str(out)))
    assert wf["metadata"]["generateName"] == "cli-pipeline-"
    assert wf["spec"]["arguments"]["parameters"] == [{"name": "msg", "value": "hi"}]


def test_tolerations_template():
    with dsl.Pipeline("t"):
        op = dsl.ContainerOp(name="download", image="busybox", command=["sh", "-c"],
                             arguments=["sleep 10; wget localhost:5678 -O /tmp/results.txt"],
                             file_outputs={"downloaded": "/tmp/results.txt"}) \
            .add_toleration(V1Toleration(effect="NoSchedule", key="gpu", operator="Equal", value="run"))
    t = op_to_template(op)
    assert t["tolerations"] == [{"effect": "NoSchedule", "key": "gpu", "operator": "Equal", "value": "run"}]
    # the reference's tolerations.yaml template, op and output names aside
    del t["name"]
    del t["outputs"]["parameters"][0]["name"]
    assert _digest(t) == _ref_digest("tolerations_template")


def test_kaniko_spec_matches_golden():
    spec = kaniko_pod_spec("default", "dockerfile", "gs://mlpipeline/kaniko_build.tar.gz",
                           "gcr.io/mlpipeline/kaniko_image:latest")
    assert _digest(spec) == _ref_digest("kaniko_basic")
    assert spec["spec"]["containers"][0]["args"][2] == "--context=gs://mlpipeline/kaniko_build.tar.gz"


def test_set_display_name_and_op_transformers():
    op1 = components.load_component_from_text("name: Component name\nimplementation:\n  container:\n"
                                              "    image: busybox\n")

    @dsl.pipeline()
    def some_pipeline():
        op1().set_display_name("Custom name")
        dsl.ContainerOp(name="sleep", image="busybox", command=["sleep 1"])
        dsl.get_pipeline_conf().op_transformers.append(lambda op: op.set_retry(5))

    wf = compiler.Compiler()._compile(some_pipeline)
    tmpls = {t["name"]: t for t in wf["spec"]["templates"]}
    assert tmpls["component-name"]["metadata"]["annotations"][
        "kubeflow.org/pipelines/task_display_name"] == "Custom name"
    for t in tmpls.values():
        if "container" in t:
            assert t["retryStrategy"]["limit"] == 5


def _typed_op():
    @dsl.component
    def a_op(field_m: {"GCSPath": {"path_type": "file", "file_type": "tsv"}}, field_o: Integer()):
        return dsl.ContainerOp(name="operator a", image="gcr.io/ml-pipeline/component-b",
                               arguments=["--field-l", field_m, "--field-o", field_o])

    return a_op


def test_type_checking_consistent_types():
    a_op = _typed_op()

    @dsl.pipeline(name="p1", description="description1")
    def my_pipeline(a: {"GCSPath": {"path_type": "file", "file_type": "tsv"}} = "good", b: Integer() = 12):
        a_op(field_m=a, field_o=b)

    compiler.Compiler().compile_to_workflow(my_pipeline, type_check=True)


def test_type_checking_inconsistent_types():
    a_op = _typed_op()

    @dsl.pipeline(name="p1", description="description1")
    def my_pipeline(a: {"GCSPath": {"path_type": "file", "file_type": "csv"}} = "good", b: Integer() = 12):
        a_op(field_m=a, field_o=b)

    with pytest.raises(InconsistentTypeException):
        compiler.Compiler().compile_to_workflow(my_pipeline, type_check=True)
    compiler.Compiler().compile_to_workflow(my_pipeline, type_check=False)


def test_type_checking_json_schema_validation():
    gcr = {"GCRPath": {"openapi_schema_validator": {"type": "string", "pattern": "^.*gcr\\.io/.*$"}}}

    @dsl.component
    def a_op(field_m: gcr, field_o: "Integer"):
        return dsl.ContainerOp(name="operator a", image="gcr.io/ml-pipeline/component-b",
                               arguments=["--field-l", field_m, "--field-o", field_o])

    @dsl.pipeline(name="p1", description="description1")
    def my_pipeline(a: gcr = "good", b: "Integer" = 12):
        a_op(field_m=a, field_o=b)

    with pytest.raises(ValueError):  # default 'good' violates the GCRPath pattern
        compiler.Compiler().compile_to_workflow(my_pipeline, type_check=True)


def test_after_dependency():
    @dsl.pipeline(name="after")
    def p():
        a = dsl.ContainerOp(name="a", image="busybox", command=["true"])
        dsl.ContainerOp(name="b", image="busybox", command=["true"]).after(a)

    wf = compiler.Compiler()._compile(p)
    dag = next(t for t in wf["spec"]["templates"] if t["name"] == "after")["dag"]["tasks"]
    assert next(t for t in dag if t["name"] == "b")["dependencies"] == ["a"]


def test_exit_handler_must_be_global():
    @dsl.pipeline(name="bad exit")
    def p():
        dsl.ContainerOp(name="x", image="busybox", command=["true"])
        with dsl.ExitHandler(dsl.ContainerOp(name="e", image="busybox", command=["true"])):
            dsl.ContainerOp(name="y", image="busybox", command=["true"])

    with pytest.raises(ValueError):
        compiler.Compiler()._compile(p)
