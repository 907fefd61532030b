"""MI355X-native drop-in for the `ctu` package surface of SenseBrain/JPD-SE that lies on the
training hot path: `ctu.models`, `ctu.trainers`, the two `ctu.utils` helpers they use
 and, of `ctu.quantizers`, the soft-to-hard vector quantizer S2HVQ.
Everything else of the reference (parsers, datasets, visualisation, the round quantizer) is out of
scope and intentionally absent."""
