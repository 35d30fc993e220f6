"""ops.kernels.index_scan_stream refuses the non-temporal row stream for every form that has none
-- the int8 image, widths 768 / 1024, the deeper rings -- before the extension is touched."""
import pytest

from codename_symbiont_amd.ops import kernels as K


class _Touched(AssertionError):
    pass


@pytest.fixture
def ext(monkeypatch):
    """The extension replaced by a recorder: its calls are listed, never run."""
    calls = []

    class Ext:
        def index_scan_stream(self, *a, **kw):
            calls.append((a, kw))

    monkeypatch.setattr(K, "hip", lambda: Ext())
    return calls


@pytest.mark.parametrize("dim,form,depth", [(384, 0, 0), (768, 0, 0), (1024, 0, 0), (768, 1, 0),
                                            (1024, 1, 0), (384, 1, 4), (384, 1, 5)])
def test_nt_is_refused_before_the_extension(monkeypatch, dim, form, depth):
    def touched():
        raise _Touched("the extension was loaded")

    monkeypatch.setattr(K, "hip", touched)
    assert not K.scan_stream_nt_ok(dim, form, depth)
    with pytest.raises(ValueError, match="non-temporal"):
        K.index_scan_stream(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, dim=dim, form=form,
                            depth=depth, nt=1)
    if dim == 384 and depth == 0:   # (the binding's defaults: dim 384, form 0 = int8)
        with pytest.raises(ValueError, match="non-temporal"):
            K.index_scan_stream(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, nt=1)


def test_nt_values_are_checked(monkeypatch):
    monkeypatch.setattr(K, "hip", lambda: (_ for _ in ()).throw(_Touched()))
    with pytest.raises(ValueError, match="nt must be 0 or 1"):
        K.index_scan_stream(dim=384, form=1, nt=2)


@pytest.mark.parametrize("depth", [0, 3])
def test_nt_passes_through_for_fp4_at_384(ext, depth):
    assert K.scan_stream_nt_ok(384, 1, depth)
    K.index_scan_stream(1, 2, 3, dim=384, form=1, depth=depth, wide=1, nt=1)
    assert ext == [((1, 2, 3), dict(dim=384, form=1, depth=depth, wide=1, nt=1))]


@pytest.mark.parametrize("dim,form", [(384, 0), (768, 1), (1024, 0)])
def test_nt_off_passes_every_form_through(ext, dim, form):
    K.index_scan_stream(7, dim=dim, form=form)
    assert ext == [((7,), dict(dim=dim, form=form, nt=0))]
