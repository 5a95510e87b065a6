"""CPU: the ctypes binding tables (serl_amd/_lib.py, serl_amd/_lib_agent.py) against include/serl_mi355.h -- every function
the header declares has exactly one table entry, with as many argtypes as the prototype has parameters."""
from serl_amd import _lib, _lib_agent


def test_every_prototype_has_one_binding_of_its_arity():
    header = _lib.exported_symbols()
    tables = (_lib.SIGNATURES, _lib_agent.SIGNATURES)
    assert len(header) >= 80
    assert not set(tables[0]) & set(tables[1]), "declared in both binding tables"
    bound = {**tables[0], **tables[1]}
    assert sorted(bound) == sorted(header), ("missing:", sorted(set(header) - set(bound)),
                                             "not in the header:", sorted(set(bound) - set(header)))
    wrong = {name: (len(bound[name]), n) for name, n in header.items() if len(bound[name]) != n}
    assert not wrong, f"argtypes / header parameter counts differ: {wrong}"
    assert not set(_lib.RESTYPES) - set(_lib.SIGNATURES) and not set(_lib_agent.RESTYPES) - set(_lib_agent.SIGNATURES)


def test_loading_the_library_applies_both_tables():
    import __graft_entry__ as ge
    ge.build()
    L = _lib.lib()
    for name, args in {**_lib.SIGNATURES, **_lib_agent.SIGNATURES}.items():
        assert list(getattr(L, name).argtypes) == args, name
