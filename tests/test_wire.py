"""Wire contract: the runtime-built messages round-trip, the rendered ``.proto`` text, the servers'
answers to unimplemented methods and the drop-in ``lms_pb2`` / ``lms_pb2_grpc`` modules."""
import hashlib
import os

import pytest

from distributed_lms_raft_llm_amd import wire
from distributed_lms_raft_llm_amd.wire import pb
from distributed_lms_raft_llm_amd.wire.schema import build_file_descriptor_proto, render_proto


def test_descriptor_is_pinned():
    """The wire contract does not drift unnoticed: the runtime-built descriptor (every message,
    field name, number, type and label, every service method and its streaming shape) serialises
    to the bytes it had when it was last compared, field for field, with the reference's
    generated descriptor.  A deliberate change of ``wire/schema.py`` updates the digest here:
    ``python -c "import hashlib; from distributed_lms_raft_llm_amd.wire.schema import build_file_descriptor_proto as b;
    print(hashlib.sha256(b().SerializeToString(deterministic=True)).hexdigest())"`` (one line)."""
    fdp = build_file_descriptor_proto()
    assert (fdp.name, fdp.package, fdp.syntax) == ("lms.proto", "lms", "proto3")
    assert (len(fdp.message_type), sum(len(m.field) for m in fdp.message_type)) == (37, 81)
    assert (len(fdp.service), sum(len(s.method) for s in fdp.service)) == (4, 21)
    digest = hashlib.sha256(fdp.SerializeToString(deterministic=True)).hexdigest()
    assert digest == "3398f7e3646b949831254d03bb77ab06355b8642ffd391d2260e00134e63b3c0"


def test_roundtrip_bytes_and_rendered_proto():
    req = pb.AppendEntriesRequest(leader=pb.TermLeaderIDPair(leaderID=3, term=7), prevLogIndex=4, prevLogTerm=6,
                                  entries=[pb.LogEntry(term=7, command='{"operation": "NoOp", "args": []}')],
                                  leaderCommit=4)
    again = pb.AppendEntriesRequest.FromString(req.SerializeToString())
    assert again == req
    text = render_proto()
    assert "rpc SendFile(stream FileChunk) returns (FileTransferResponse);" in text
    assert "repeated DataEntry entries = 3;" in text


def test_unimplemented_methods_answer_unimplemented(tmp_path):
    import grpc

    from lms_harness import Cluster

    c = Cluster(1, tmp_path)
    try:
        c.wait_leader()
        ch = wire.channel(c.addrs[1])
        with pytest.raises(grpc.RpcError) as ei:
            wire.Stub("FileTransferService", ch).ReplicateData(pb.ReplicateDataRequest(), timeout=5)
        assert ei.value.code() == grpc.StatusCode.UNIMPLEMENTED
        # the RaftService debug KV API is implemented on top of the log
        rs = wire.Stub("RaftService", ch)
        assert rs.SetVal(pb.SetValRequest(key="k", value="v"), timeout=5).verdict
        assert rs.GetVal(pb.GetValRequest(key="k"), timeout=5).value == "v"
        gl = rs.GetLeader(pb.GetLeaderRequest(), timeout=5)
        assert gl.nodeId == 1 and gl.nodeAddress == c.addrs[1]
        ch.close()
    finally:
        c.close()


def test_dropin_generated_modules():
    """Top-level lms_pb2 / lms_pb2_grpc: the generated modules' API (stubs, servicer bases with
    UNIMPLEMENTED defaults, add_*_to_server, experimental static calls)."""
    import importlib.util
    from concurrent import futures

    import grpc

    from distributed_lms_raft_llm_amd.wire import lms_pb2, lms_pb2_grpc

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("lms_pb2", "lms_pb2_grpc"):  # the top-level shims re-export them (loaded by path:
        spec = importlib.util.spec_from_file_location(f"_shim_{name}", os.path.join(root, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)  # another test may have cached the reference's)
        spec.loader.exec_module(mod)
        assert hasattr(mod, "LoginRequest" if name == "lms_pb2" else "LMSStub")
    assert lms_pb2.DESCRIPTOR.package == "lms"

    class Tutor(lms_pb2_grpc.Tutoring):  # the reference tutoring server subclasses this class
        def GetLLMAnswer(self, request, context):
            return lms_pb2.QueryResponse(success=True, response="echo " + request.query)

    srv = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    lms_pb2_grpc.add_TutoringServicer_to_server(Tutor(), srv)
    lms_pb2_grpc.add_RaftServiceServicer_to_server(lms_pb2_grpc.RaftServiceServicer(), srv)
    port = srv.add_insecure_port("127.0.0.1:0")
    srv.start()
    try:
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            r = lms_pb2_grpc.TutoringStub(ch).GetLLMAnswer(lms_pb2.QueryRequest(token="t", query="q"), timeout=5)
            assert r.success and r.response == "echo q"
            with pytest.raises(grpc.RpcError) as e:
                lms_pb2_grpc.RaftServiceStub(ch).WhoIsLeader(lms_pb2.Empty(), timeout=5)
            assert e.value.code() == grpc.StatusCode.UNIMPLEMENTED
        r = lms_pb2_grpc.Tutoring.GetLLMAnswer(lms_pb2.QueryRequest(query="s"), f"127.0.0.1:{port}", timeout=5)
        assert r.response == "echo s"
    finally:
        srv.stop(0)
