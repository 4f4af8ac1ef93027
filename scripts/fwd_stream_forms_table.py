"""profiles/fwd_stream_forms_parity.txt from a parity log (tests/conftest.py parity_log: the file SSC_PARITY_LOG names, or its
default): per case and launch of tests/test_gpu_fwd_stream_forms.py the plan ssc_conv_stream_plan reported ({kernel,
instantiation, tiles, workgroups}; '-' where none of the seven streaming kernels takes the launch) and the worst err / bound
ratio, then the worst ratio per kernel and instantiation.
python scripts/fwd_stream_forms_table.py <parity.jsonl> > <table>"""
import json
import sys

recs = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
recs = [r for r in recs if r['test'] == 'fwd_stream_forms']
worst = {}
for r in recs:
    c = r['config']
    key = (c['case'], c['rider'])
    if key not in worst or r['ratio'] > worst[key]['ratio']:
        worst[key] = r
print('%-26s %-5s %-22s %-4s %-4s %6s %6s %5s  %-9s %-9s %-9s' %
      ('case', 'rider', 'kernel', 'inst', 'walk', 'tiles', 'wgs', 'K', 'err/bound', 'err', 'bound'))
for (case, rider), r in worst.items():
    c, p = r['config'], r['plan']
    print('%-26s %-5s %-22s %-4s %-4d %6s %6s %5d  %.3e %.3e %.3e' %
          (case, rider, c['kernel'], '-' if p is None else p[1], c['walk'], '-' if p is None else p[2], '-' if p is None else p[3],
           r['K'], r['ratio'], r['max_abs_err'], r['bound']))
forms = {}
for r in worst.values():
    c = r['config']
    key = (c['kernel'], c['inst'])
    if key not in forms or r['ratio'] > forms[key]['ratio']:
        forms[key] = r
print()
for (kernel, inst), r in sorted(forms.items(), key=lambda kv: (kv[0][0], -1 if kv[0][1] is None else kv[0][1])):
    n = sum(1 for x in worst.values() if (x['config']['kernel'], x['config']['inst']) == (kernel, inst))
    print('%-22s instantiation %-4s %2d launches, worst err/bound %.3e (%s)' %
          (kernel, '-' if inst is None else inst, n, r['ratio'], r['config']['case']))
